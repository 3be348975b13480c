"""Per-pixel sample masks and the adaptive loop on the device: the mask kernel and its
compaction (surf_adaptive_mask_image, surf_mask_from_noise), masked renders
(surf_set_pixel_mask), the loop (surf_render_adaptive) and the weighted packing, against
the oracle's per-sample radiance and the numpy restatements of tests/test_adaptive_host.py.

Bar: bit-exact, planes compared as uint32 words, masks, lists and counters as integers.
The expected values never come from the code under test.

No rendered frame exceeds 100 x 37; the one large case, 2048 x 600, is two synthetic planes
through the mask kernels alone (4,800 blocks behind the cross-block scan), no render.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import surf_amd
from surf_amd import ShardSpec
from test_adaptive_host import (LOOP, check_mask, frame_planted, loop_case, np_add_frame, np_mask, np_pack_weighted, weighted_records)
from test_denoise_host import assert_images_equal
from test_gpu_aov import read_pfm
from test_sampled_host import W, H, np_noise, np_squares, oracle_samples

pytestmark = pytest.mark.gpu
F = np.float32
SURF_ERR_INVALID = -1
COUNTERS = ("samples", "n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def renderer(scene, w=W, h=H, squares=True, **kw):
    r = surf_amd.Renderer(scene, w, h, **kw)
    if squares:
        r.set_sample_squares(True)
    return r


def assert_words_equal(got, want, what):
    assert_images_equal(np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32), what)


def np_masked(samples, schedule, h, w):
    """(A, Q) after the schedule's renders: [(mask or None, first, count), ...] of spp-1 frames."""
    A, Q = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    for mask, first, count in schedule:
        m = np.ones((h, w), np.uint8) if mask is None else mask
        for j in range(first, first + count):
            A, Q = np_add_frame(A, Q, samples[j], m)
    return A, Q


def random_mask(h, w, seed=7):
    return (np.random.default_rng(seed).random((h, w)) < 0.5).astype(np.uint8)


@pytest.fixture(scope="module")
def ctx(product_scene):
    """A context for the image forms (shared; the tests leave its accumulator alone)."""
    r = surf_amd.Renderer(product_scene, 8, 8)
    yield r
    r.close()


# ---- 1. the mask kernel -----------------------------------------------------------------------------

def test_mask_image_matches_numpy_and_the_host_twin(ctx):
    check_mask(ctx.adaptive_mask_image, "device")
    A, Q = frame_planted()
    for d in (0, 1, 2):
        p = dict(threshold=0.3, min_samples=4, max_samples=8, dilate=d)
        (gm, gl), (hm, hl) = ctx.adaptive_mask_image(A, Q, **p), surf_amd.adaptive_mask_image_host(A, Q, **p)
        assert np.array_equal(gm, hm) and np.array_equal(gl, hl), d


def test_mask_image_large(ctx):
    """2048 x 600 synthetic planes: 1,228,800 pixels, 4,800 compaction blocks, 64 x 75 tiles."""
    rng = np.random.default_rng(20)
    h, w = 600, 2048
    n = rng.integers(0, 41, (h, w)).astype(np.float32)
    mean = rng.random((h, w, 3), dtype=np.float32)
    A = np.concatenate([mean * n[..., None], n[..., None]], -1).astype(np.float32)
    Q = (rng.random((h, w, 4), dtype=np.float32) * F(2.0)) * n[..., None]
    quiet = rng.random((h, w)) < 0.9                           # most pixels: squares that match the mean, so t is about 0
    lb = (F(0.2126) * mean[..., 0] + F(0.7152) * mean[..., 1]) + F(0.0722) * mean[..., 2]
    Q[..., 3] = np.where(quiet, lb * lb * n, Q[..., 3])
    for p in (dict(threshold=0.05, min_samples=8, max_samples=36, dilate=1), dict(threshold=0.05, min_samples=8, max_samples=36, dilate=0),
              dict(threshold=0.2, min_samples=2, max_samples=30, dilate=2)):
        want_mask, want_list, _ = np_mask(A, Q, **p)
        assert 0.05 * h * w < len(want_list) < 0.95 * h * w, (p, len(want_list))
        mask, lst = ctx.adaptive_mask_image(A, Q, **p)
        assert np.array_equal(mask, want_mask), (p, int((mask != want_mask).sum()))
        assert len(lst) == len(want_list) and np.array_equal(lst, want_list), p
    none = ctx.adaptive_mask_image(A, Q, threshold=0.05, min_samples=2, max_samples=2)       # nothing below the cap of 2 but n < 2
    assert np.array_equal(none[0], np_mask(A, Q, threshold=0.05, min_samples=2, max_samples=2)[0])


def test_image_path_needs_no_scene_and_no_plane():
    lib = surf_amd.load()
    A, Q = frame_planted()
    h, w = A.shape[:2]
    hnd = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(hnd)) == 0
    try:
        p = surf_amd.adaptive_mask_params(threshold=0.3, min_samples=4, max_samples=8)
        mask, n = np.zeros((h, w), np.uint8), C.c_uint32()
        assert lib.surf_mask_from_noise(hnd, C.byref(p), C.byref(n)) == SURF_ERR_INVALID                 # the plane is off
        assert lib.surf_adaptive_mask_image(hnd, w, h, A.ctypes.data, Q.ctypes.data, C.byref(p), mask.ctypes.data, None, C.byref(n)) == 0
        want = np_mask(A, Q, threshold=0.3, min_samples=4, max_samples=8)
        assert np.array_equal(mask, want[0]) and n.value == len(want[1])
        assert lib.surf_adaptive_mask_image(hnd, 0, h, A.ctypes.data, Q.ctypes.data, C.byref(p), mask.ctypes.data, None, C.byref(n)) == SURF_ERR_INVALID
        bad = surf_amd.adaptive_mask_params(dilate=3)
        assert lib.surf_adaptive_mask_image(hnd, w, h, A.ctypes.data, Q.ctypes.data, C.byref(bad), mask.ctypes.data, None, C.byref(n)) == SURF_ERR_INVALID
        got, cnt = np.zeros((8, 8), np.uint8), C.c_uint32()
        assert lib.surf_get_pixel_mask(hnd, got.ctypes.data, C.byref(cnt)) == 0 and got.all() and cnt.value == 64   # the context's mask is left alone
    finally:
        lib.surf_destroy(hnd)


# ---- 2. masked renders ------------------------------------------------------------------------------

def test_random_mask(product_scene):
    samples, _, _ = oracle_samples(8)
    mask = random_mask(H, W)
    assert 0.4 * W * H < mask.sum() < 0.6 * W * H
    A, Q = np_masked(samples, [(mask, 0, 8)], H, W)
    r = renderer(product_scene)
    try:
        r.set_pixel_mask(mask)
        got_mask, count = r.pixel_mask()
        assert np.array_equal(got_mask, mask) and count == int(mask.sum())
        r.render(8, 0)
        acc, sq = r.accumulator(), r.sample_squares()
        assert_words_equal(acc, A, "accumulator under a random mask")           # inactive records: all-zero words
        assert_words_equal(sq, Q, "squares under a random mask")
        assert not acc[mask == 0].view(np.uint32).any() and not sq[mask == 0].view(np.uint32).any()
        assert (acc[mask != 0][:, 3] == 8.0).all()
        assert r.stats()["samples"] == 8 * int(mask.sum())
        assert r.debug_issue_order()[1] == 0                                      # masked streams have no permuted head
    finally:
        r.close()


def test_row_band_matches_the_oracles_row_render(oracle_scene, product_scene):
    w, h, r0, r1, frames = 32, 24, 7, 16, 3
    mask = np.zeros((h, w), np.uint8)
    mask[r0:r1] = 1
    oracle.set_zero_cutoff(False)
    c, _, _ = oracle_scene.render(w, h, frames, rows=(r0, r1))
    oracle.set_zero_cutoff(True)
    try:
        c2, cnt, _ = oracle_scene.render(w, h, frames, rows=(r0, r1))
    finally:
        oracle.set_zero_cutoff(False)
    assert np.array_equal(c.view(np.uint32), c2.view(np.uint32)), "cutoff changed the oracle's radiance"
    r = surf_amd.Renderer(product_scene, w, h)
    try:
        r.set_pixel_mask(mask)
        r.render(frames, 0)
        acc, st = r.accumulator(), r.stats()
    finally:
        r.close()
    assert_words_equal(acc[r0:r1], c, "the band's rows against the oracle's row-restricted render")
    assert not acc[:r0].view(np.uint32).any() and not acc[r1:].view(np.uint32).any()
    assert st["samples"] == frames * (r1 - r0) * w
    for k in COUNTERS[1:]:
        assert st[k] == cnt[k], (k, st[k], cnt[k])


def test_all_ones_is_no_mask(product_scene):
    got = {}
    for masked in (False, True):
        r = renderer(product_scene)
        try:
            if masked:
                r.set_pixel_mask(np.ones((H, W), np.uint8))
            r.render(8, 0)
            st = r.stats()
            got[masked] = (r.accumulator(), r.sample_squares(), [st[k] for k in COUNTERS + ("iterations",)], r.debug_issue_order(), r.pixel_mask()[1])
        finally:
            r.close()
    assert_words_equal(got[True][0], got[False][0], "accumulator, all-ones mask against none")
    assert_words_equal(got[True][1], got[False][1], "squares, all-ones mask against none")
    assert got[True][2:] == got[False][2:], (got[True][2:], got[False][2:])
    assert got[False][3][0] > 0 and got[False][3][1] == 8 and got[False][4] == W * H           # the heavy-pixels-first order, both


def test_all_zero_does_nothing(product_scene):
    samples, _, _ = oracle_samples(2)
    A, Q = np_squares(samples)
    r = renderer(product_scene)
    try:
        r.render(2, 0)
        before = r.stats()
        r.set_pixel_mask(np.zeros((H, W), np.uint8))
        assert r.pixel_mask()[1] == 0 and not r.pixel_mask()[0].any()
        assert surf_amd.load().surf_render(r.handle, 4, 2, 0, 1) == 0
        after = r.stats()
        assert [after[k] for k in COUNTERS] == [before[k] for k in COUNTERS]
        assert_words_equal(r.accumulator(), A, "accumulator after an all-zero render")
        assert_words_equal(r.sample_squares(), Q, "squares after an all-zero render")
        assert np.array_equal(r.finalize_rgba8(), surf_amd.pack_rgba8(A, 2).reshape(H, W))       # the frame count did not move
    finally:
        r.close()


def test_last_pixel_alone(product_scene):
    samples, _, _ = oracle_samples(8)
    mask = np.zeros((H, W), np.uint8)
    mask[-1, -1] = 1
    A, Q = np_masked(samples, [(mask, 0, 8)], H, W)
    r = renderer(product_scene)
    try:
        r.set_pixel_mask(mask)
        r.render(8, 0)
        assert_words_equal(r.accumulator(), A, "one active pixel, the frame's last")
        assert_words_equal(r.sample_squares(), Q, "squares: one active pixel")
        assert r.stats()["samples"] == 8
    finally:
        r.close()


# ---- 3. streams -------------------------------------------------------------------------------------

def test_mask_changes_between_streams(product_scene):
    samples, _, _ = oracle_samples(10)
    mask = random_mask(H, W, 11)
    A, Q = np_masked(samples, [(None, 0, 4), (mask, 4, 4), (None, 8, 2)], H, W)
    r = renderer(product_scene)
    try:
        r.render(4, 0)
        r.set_pixel_mask(mask)
        r.render(4, 4)
        r.set_pixel_mask(None)
        r.render(2, 8)
        assert_words_equal(r.accumulator(), A, "unmasked, masked, unmasked")
        assert_words_equal(r.sample_squares(), Q, "squares: unmasked, masked, unmasked")
        assert r.stats()["samples"] == 6 * W * H + 4 * int(mask.sum())
        assert np.array_equal(np.unique(A[..., 3]), [6.0, 10.0])
    finally:
        r.close()


def test_ring_reuse(product_scene):
    w, h = 32, 24
    samples, _, _ = oracle_samples(10, w, h)
    mask = random_mask(h, w, 3)
    A, Q = np_masked(samples, [(mask, 0, 10)], h, w)
    r = renderer(product_scene, w, h, frame_batch=4)
    try:
        r.set_pixel_mask(mask)
        r.render(10, 0)
        assert r.stats()["frame_window"] == 4                                    # 10 passes reuse the 4 slots
        assert_words_equal(r.accumulator(), A, "10 masked frames in a window of 4")
        assert_words_equal(r.sample_squares(), Q, "squares: 10 masked frames in a window of 4")
    finally:
        r.close()


def test_drop_in_loop(product_scene):
    samples, _, _ = oracle_samples(16)
    mask = random_mask(H, W, 5)
    A, Q = np_masked(samples, [(mask, 0, 16)], H, W)
    r = renderer(product_scene)
    try:
        r.set_pixel_mask(mask)
        for j in range(16):
            r.render(1, j)
        assert_words_equal(r.accumulator(), A, "sixteen one-frame masked calls")
        assert_words_equal(r.sample_squares(), Q, "squares: sixteen one-frame masked calls")
        assert r.stats()["samples"] == 16 * int(mask.sum())
    finally:
        r.close()


def test_multi_sample_frames(oracle_scene, product_scene):
    """Chains through chainNext and the drain: 3 frames of 4 samples against the oracle's."""
    want, _, _ = oracle_scene.render(W, H, 3, spp=4)
    mask = random_mask(H, W, 9)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        r.set_pixel_mask(mask)
        r.render(3, 0, spp=4)
        acc = r.accumulator()
        assert r.stats()["samples"] == 12 * int(mask.sum())
    finally:
        r.close()
    assert_words_equal(acc, np.where(mask[..., None] != 0, want, F(0.0)), "3 masked frames of 4 samples")


SHARDS = [ShardSpec(k, 3, 2) for k in range(3)]


def test_row_shards(product_scene):
    samples, _, _ = oracle_samples(8)
    mask = random_mask(H, W, 13)
    A, Q = np_masked(samples, [(None, 0, 4), (mask, 4, 4)], H, W)
    A4, Q4 = np_squares(samples[:4])
    p = dict(threshold=0.5, min_samples=4, max_samples=36)
    rs = [renderer(product_scene, shard=s) for s in SHARDS]
    try:
        for r in rs:
            r.render(4, 0)
        # the rule per shard: pointwise with dilate 0, refused with a dilation
        want0 = np_mask(A4, Q4, dilate=0, **p)[0]
        parts = []
        for r in rs:
            n = r.mask_from_noise(dilate=0, **p)
            m, cnt = r.pixel_mask()
            assert cnt == n == int(m.sum())
            parts.append(np.repeat(m[..., None].astype(np.float32), 4, -1))
            with pytest.raises(surf_amd.SurfError) as e:
                r.mask_from_noise(dilate=1, **p)
            assert e.value.code == SURF_ERR_INVALID and "surf_adaptive_mask_image" in str(e.value)
            assert r.pixel_mask()[1] == n                                          # a refused call leaves the mask
        assert np.array_equal(surf_amd.assemble_shards(W, H, parts, SHARDS)[..., 0], want0.astype(np.float32))
        assert 0 < want0.sum() < W * H
        # per-shard masks cut from one frame mask, assembled
        for r in rs:
            r.set_pixel_mask(mask[r.rows])
            r.render(4, 4)
        assert_words_equal(surf_amd.assemble_shards(W, H, [r.accumulator() for r in rs], SHARDS), A, "accumulator from three masked row shards")
        assert_words_equal(surf_amd.assemble_shards(W, H, [r.sample_squares() for r in rs], SHARDS), Q, "squares from three masked row shards")
    finally:
        for r in rs:
            r.close()


def test_clear_resets_the_mask(product_scene):
    samples, _, _ = oracle_samples(2)
    A, Q = np_squares(samples)
    r = renderer(product_scene)
    try:
        r.set_pixel_mask(random_mask(H, W, 17))
        r.render(2, 0)
        r.clear_accumulator()
        m, n = r.pixel_mask()
        assert m.all() and n == W * H
        r.render(2, 0)
        assert_words_equal(r.accumulator(), A, "after clear_accumulator: every pixel again")
        r.set_pixel_mask(random_mask(H, W, 17))
        r.set_camera(product_scene.camera(W, H))                                  # camera updates keep it
        assert r.pixel_mask()[1] == int(random_mask(H, W, 17).sum())
    finally:
        r.close()


# ---- 4. the mask from the context's planes, the loop -----------------------------------------------

def test_mask_from_noise_on_the_context(product_scene):
    samples, _, _ = oracle_samples(16)
    A, Q = np_squares(samples[:8])
    r = renderer(product_scene)
    try:
        r.render(8, 0)
        for p in (dict(threshold=0.5, min_samples=4, max_samples=36, dilate=1), dict(threshold=0.8, min_samples=4, max_samples=36, dilate=2),
                  dict(threshold=0.5, min_samples=4, max_samples=36, dilate=0)):
            want_mask, want_list, _ = np_mask(A, Q, **p)
            assert 0 < len(want_list) < W * H
            assert r.mask_from_noise(**p) == len(want_list), p
            m, n = r.pixel_mask()
            assert np.array_equal(m, want_mask) and n == len(want_list), p
        assert r.mask_from_noise(threshold=0.5, min_samples=9, max_samples=36) == W * H          # below min_samples: every pixel, no mask
        assert r.mask_from_noise(threshold=0.5, min_samples=4, max_samples=8) == 0               # at max_samples: none
        assert not r.pixel_mask()[0].any()
        # the device-built list drives a render: the last mask with pixels on both sides
        p = dict(threshold=0.5, min_samples=4, max_samples=36, dilate=1)
        want_mask = np_mask(A, Q, **p)[0]
        r.mask_from_noise(**p)
        r.render(8, 8)
        A2, Q2 = np_masked(samples, [(None, 0, 8), (want_mask, 8, 8)], H, W)
        assert_words_equal(r.accumulator(), A2, "8 frames under the device-built mask")
        assert_words_equal(r.sample_squares(), Q2, "squares: 8 frames under the device-built mask")
    finally:
        r.close()


def test_render_adaptive_matches_the_restatement(product_scene):
    want = loop_case()
    r = renderer(product_scene)
    try:
        got = r.render_adaptive(**LOOP)
        assert got["round_active"] == want["round_active"], (got["round_active"], want["round_active"])
        assert (got["rounds"], got["frames"], got["samples"], got["active_last"]) == (want["rounds"], want["frames"], want["samples"], want["active_last"])
        assert_words_equal(r.accumulator(), want["acc"], "render_adaptive: accumulator")
        assert_words_equal(r.sample_squares(), want["squares"], "render_adaptive: squares")
        m, n = r.pixel_mask()
        assert np.array_equal(m, want["mask"]) and n == want["active_last"]                        # the final mask stays set
        assert (got["noise"]["pixels"], got["noise"]["above"]) == (want["noise"]["pixels"], want["noise"]["above"])
        assert F(got["noise"]["max_error"]).view(np.uint32) == F(want["noise"]["max_error"]).view(np.uint32)
        assert r.stats()["samples"] == want["samples"]
        with pytest.raises(surf_amd.SurfError) as e:                                                # the accumulator holds samples
            r.render_adaptive(**LOOP)
        assert e.value.code == SURF_ERR_INVALID
        r.clear_accumulator()
        short = r.render_adaptive(round_cap=2, **LOOP)                                              # round_cap bounds what is written
        assert short["rounds"] == want["rounds"] and short["round_active"] == want["round_active"][:2]
    finally:
        r.close()
    plain = surf_amd.Renderer(product_scene, 33, 9)
    try:
        with pytest.raises(surf_amd.SurfError) as e:                                                # squares off
            plain.render_adaptive(**LOOP)
        assert e.value.code == SURF_ERR_INVALID
    finally:
        plain.close()


def test_render_adaptive_stops_when_nothing_is_active(product_scene):
    """A threshold nothing exceeds: the loop ends after min_samples frames, before max_samples."""
    samples, _, _ = oracle_samples(4)
    A, Q = np_squares(samples)
    r = renderer(product_scene)
    try:
        got = r.render_adaptive(threshold=1e6, min_samples=4, max_samples=36, batch=4)
        assert (got["rounds"], got["frames"], got["active_last"], got["samples"], got["round_active"]) == (0, 4, 0, 4 * W * H, [])
        assert_words_equal(r.accumulator(), A, "render_adaptive that stops at min_samples")
    finally:
        r.close()


# ---- 5. the weighted packing, the example -----------------------------------------------------------

def test_finalize_weighted(product_scene):
    samples, _, _ = oracle_samples(8)
    mask = random_mask(H, W, 21)
    A, _ = np_masked(samples, [(mask, 0, 3), (None, 3, 5)], H, W)
    r = renderer(product_scene, squares=False)
    try:
        r.set_pixel_mask(mask)
        r.render(3, 0)
        r.set_pixel_mask(None)
        r.render(5, 3)
        for display in (False, True):
            assert np.array_equal(r.finalize_weighted(display).reshape(-1), np_pack_weighted(A, display)), display
        r.clear_accumulator()
        assert not r.finalize_weighted().any()                                                     # w = 0 everywhere
    finally:
        r.close()
    rec = weighted_records()
    assert np.array_equal(surf_amd.pack_rgba8_weighted(rec, True), np_pack_weighted(rec, True))


def test_cpp_example_matches_python(product_scene, tmp_path):
    exe = os.path.join(surf_amd._PKG, "build", "render_denoised")
    word_rows = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    prefix = str(tmp_path / "ad")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "2", prefix, "24"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = renderer(product_scene)
    try:
        got = r.render_adaptive(max_samples=24)
        acc = r.accumulator()
    finally:
        r.close()
    n = acc[..., 3]
    mean = acc[..., :3] * np.where(n > 0, F(1.0) / n, F(0.0)).astype(np.float32)[..., None]
    assert np.array_equal(word_rows(read_pfm(prefix + "_adaptive.pfm")), word_rows(mean))
    assert np.array_equal(word_rows(read_pfm(prefix + "_counts.pfm")), word_rows(np.repeat(n[..., None], 3, -1)))
    assert f'"adaptive_frames": {got["frames"]}' in run.stdout and f'"adaptive_samples": {got["samples"]}' in run.stdout
    plain = str(tmp_path / "plain")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, "33", "9", "2", plain], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and not os.path.exists(plain + "_adaptive.pfm")
