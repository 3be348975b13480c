"""The per-sample second moments on the device: the squares plane k_accumulate keeps
(surf_set_sample_squares), the sample-variance-guided filter (surf_denoise_sampled*)
and the noise estimate (surf_noise_*), against the oracle's per-sample radiance and
the numpy restatements of tests/test_sampled_host.py.

Bar: bit-exact, planes and images compared as uint32 words.  The expected values
never come from the code under test: the squares are summed in float32 numpy from
the oracle's spp-1 frames, the images are np_sampled's and np_noise's of those.

No frame exceeds 100 x 37: 3,700 pixels, no multiple of the 256-thread block nor of
the 32 x 8 tile.
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
from test_sampled_host import (PLANTED, PLANTED_INVALID, RULES_A, RULES_Q, W, H, assert_errors_equal, frame_a, frame_c, lum, noise_threshold,
                               np_noise, np_sampled, np_squares, oracle_samples)

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


@pytest.fixture(scope="module")
def rendered_a(product_scene):
    """A context after render(16, 0) at 100 x 37 with squares on (shared; the tests only read it)."""
    r = renderer(product_scene)
    r.render(16, 0)
    yield r
    r.close()


_want = {}


def sampled_a(**params):
    """np_sampled of frame A, computed once per parameter set."""
    key = tuple(sorted(params.items()))
    if key not in _want:
        A, Q, planes, _ = frame_a()
        _want[key] = np_sampled(A, Q, planes, **params)[:2]
    return _want[key]


def assert_words_equal(got, want, what):
    assert_images_equal(np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32), what)


# ---- 1. the squares plane ----------------------------------------------------------------------

def test_squares_bitexact(rendered_a):
    A, Q, _, _ = frame_a()
    assert_words_equal(rendered_a.sample_squares(), Q, "squares, 16 frames at 100 x 37")
    assert_words_equal(rendered_a.accumulator(), A, "accumulator, 16 frames at 100 x 37")


@pytest.mark.parametrize("side", [8, 4])
def test_reset_prologue_case(product_scene, side):
    """A launch that accumulates `count` passes resets count x 32 completion stripes, with
    threads past the last pixel where that exceeds the pixel count.  8 x 8, 40 frames: 64
    pixels, so any launch of 3 or more passes -- how many passes a launch takes is the
    host's batching, which nothing here pins.  4 x 4: 16 pixels, fewer than the 32 stripes
    of a single pass, so every launch has such threads whatever the batching."""
    samples, _, _ = oracle_samples(40, side, side)
    A, Q = np_squares(samples)
    r = renderer(product_scene, side, side)
    try:
        r.render(40, 0)
        assert_words_equal(r.sample_squares(), Q, f"squares, 40 frames at {side} x {side}")
        assert_words_equal(r.accumulator(), A, f"accumulator, 40 frames at {side} x {side}")
    finally:
        r.close()


def test_ring_reuse(product_scene):
    samples, _, _ = oracle_samples(10, 32, 24)
    A, Q = np_squares(samples)
    got = {}
    for batch in (4, None):
        r = renderer(product_scene, 32, 24, frame_batch=batch)
        try:
            r.render(10, 0)
            got[batch] = (r.sample_squares(), r.accumulator(), r.stats()["frame_window"])
        finally:
            r.close()
    assert got[4][2] == 4 and got[None][2] > 10, (got[4][2], got[None][2])       # 10 passes reuse the 4 slots
    assert_words_equal(got[4][0], got[None][0], "squares: a window of 4 against the default window")
    assert_words_equal(got[4][0], Q, "squares, 10 frames at 32 x 24")
    assert_words_equal(got[4][1], A, "accumulator, 10 frames at 32 x 24")


def test_drop_in_loop(product_scene):
    A, Q, _, _ = frame_a()
    r = renderer(product_scene)
    try:
        for j in range(16):
            r.render(1, j)
        assert_words_equal(r.sample_squares(), Q, "squares, sixteen one-frame calls")
        assert_words_equal(r.accumulator(), A, "accumulator, sixteen one-frame calls")
    finally:
        r.close()


def test_neutral_to_the_stream(product_scene, rendered_a):
    r = renderer(product_scene, squares=False)
    try:
        r.render(16, 0)
        assert_words_equal(r.accumulator(), rendered_a.accumulator(), "accumulator, squares off against on")
        off, on = r.stats(), rendered_a.stats()
        assert [off[k] for k in COUNTERS] == [on[k] for k in COUNTERS]
        with pytest.raises(surf_amd.SurfError) as e:
            r.sample_squares()
        assert e.value.code == SURF_ERR_INVALID
    finally:
        r.close()


def test_lifecycle(product_scene):
    r = surf_amd.Renderer(product_scene, 33, 9)
    dev_err = lambda f, *a, **k: pytest.raises(surf_amd.SurfError, f, *a, **k).value.code
    try:
        for call in (r.sample_squares, r.denoise_sampled, r.noise_estimate):        # off: every context form refuses
            assert dev_err(call) == SURF_ERR_INVALID
        r.render(2, 0)
        assert dev_err(r.set_sample_squares, True) == SURF_ERR_INVALID            # samples present: their squares are lost
        r.clear_accumulator()
        r.set_sample_squares(True)
        assert not r.sample_squares().any()
        r.render(3, 0)
        samples, _, _ = oracle_samples(3, 33, 9)
        assert_words_equal(r.sample_squares(), np_squares(samples)[1], "squares after clear + enable")
        assert dev_err(r.set_sample_squares, False) == SURF_ERR_INVALID
        r.clear_accumulator()
        assert not r.sample_squares().any() and not r.accumulator().any()
        r.render(3, 0)
        assert_words_equal(r.sample_squares(), np_squares(samples)[1], "squares after a second clear")
        r.clear_accumulator()
        r.set_sample_squares(False)                                                # keeps the allocation, stops the sums
        r.render(3, 0)
        assert dev_err(r.sample_squares) == SURF_ERR_INVALID
        r.clear_accumulator()
        r.set_sample_squares(True)
        assert not r.sample_squares().any()
    finally:
        r.close()


def test_multi_sample_frames(product_scene):
    """The per-sample radiance of a chained frame is not the oracle's to give: invariants only."""
    got = {}
    for on in (True, False):
        r = renderer(product_scene, squares=on)
        try:
            r.render(4, 0, spp=4)
            got[on] = (r.accumulator(), r.sample_squares() if on else None)
        finally:
            r.close()
    A, Q = got[True]
    assert_words_equal(A, got[False][0], "accumulator of 4 frames of 4 samples, squares on against off")
    assert (A[..., 3] == 16.0).all()
    assert np.isfinite(Q).all() and (Q >= 0.0).all() and (Q[..., 3] > 0.0).sum() > 0.9 * W * H
    lb = lum(A[..., :3].astype(np.float64))
    assert (16.0 * Q[..., 3].astype(np.float64) >= lb * lb * (1.0 - 1e-4)).all()      # Cauchy-Schwarz; 16 f32 additions err by < 16 * 2^-24
    for k in range(3):
        a = A[..., k].astype(np.float64)
        assert (16.0 * Q[..., k].astype(np.float64) >= a * a * (1.0 - 1e-4)).all(), k


SHARDS = [ShardSpec(k, 3, 2) for k in range(3)]


@pytest.fixture(scope="module")
def rendered_shards(product_scene):
    rs = [renderer(product_scene, shard=s) for s in SHARDS]
    for r in rs:
        r.render(16, 0)
    yield rs
    for r in rs:
        r.close()


def test_row_shards(rendered_shards):
    A, Q, _, _ = frame_a()
    parts = [r.sample_squares() for r in rendered_shards]
    assert sum(len(p) for p in parts) == H
    assert_words_equal(surf_amd.assemble_shards(W, H, parts, SHARDS), Q, "squares assembled from three row shards")
    assert_words_equal(surf_amd.assemble_shards(W, H, [r.accumulator() for r in rendered_shards], SHARDS), A, "accumulator from three row shards")


# ---- 2. the filter ------------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", ["2", "0", "16"])
def test_filter_parity(product_scene, monkeypatch, lds):
    monkeypatch.setenv("SURF_DENOISE_LDS", lds)
    A, Q, planes, _ = frame_a()
    r = renderer(product_scene)
    try:
        r.render(16, 0)
        for params in ({}, dict(iterations=2, demodulate=0)):
            want_out, want_var = sampled_a(**params)
            assert_images_equal(r.denoise_sampled(**params), want_out, f"denoise_sampled {params}, SURF_DENOISE_LDS={lds}")
            ms = r.debug_sampled_time()
            n = params.get("iterations", 5)
            assert all(v > 0.0 for v in ms[:n + 1]) and not any(ms[n + 1:]), ms
            out, var = r.denoise_sampled_image(r.accumulator(), r.sample_squares(), r.aov(), **params)
            assert_images_equal(out, want_out, f"denoise_sampled_image {params}: image")
            assert_images_equal(var, want_var, f"denoise_sampled_image {params}: variance")
        assert_images_equal(r.denoise_sampled(), surf_amd.denoise_sampled_image_host(A, Q, planes)[0], "device vs host twin")
    finally:
        r.close()


def test_image_path_needs_no_scene_and_no_plane():
    lib = surf_amd.load()
    A, Q, planes, _ = frame_a()
    want_out, want_var = sampled_a()
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        w, hh, a = surf_amd._sampled_planes(A, Q, planes)
        out, var = np.zeros((hh, w, 4), np.float32), np.zeros((hh, w, 4), np.float32)
        sp = surf_amd.svgf_params()
        ptr = [x.ctypes.data for x in a]
        assert lib.surf_denoise_sampled(h, C.byref(sp), out.ctypes.data) == SURF_ERR_INVALID         # the plane is off
        assert lib.surf_denoise_sampled_image(h, w, hh, *ptr, C.byref(sp), out.ctypes.data, var.ctypes.data) == 0
        assert_images_equal(out, want_out, "context without a scene: image")
        assert_images_equal(var, want_var, "context without a scene: variance")
        assert lib.surf_denoise_sampled_image(h, 0, hh, *ptr, C.byref(sp), out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID
        assert lib.surf_denoise_sampled_image(h, w, hh, ptr[0], None, *ptr[2:], C.byref(sp), out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID
        bad = surf_amd.svgf_params(iterations=7)
        assert lib.surf_denoise_sampled_image(h, w, hh, *ptr, C.byref(bad), out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID
        assert lib.surf_set_sample_squares(h, 1) == 0
        assert lib.surf_denoise_sampled(h, C.byref(sp), out.ctypes.data) == -4                         # SURF_ERR_NO_SCENE
    finally:
        lib.surf_destroy(h)


def test_planted_records_take_the_branches_on_the_device(rendered_a):
    """Frame C (no sample, one sample, t < 0, NaN squares, invalid pixels) and the hand-made
    noise records through the device's own compilation of the per-pixel functions."""
    A, Q, planes, hit = frame_c()
    for params in ({}, dict(iterations=1, demodulate=0)):
        want_out, want_var, cnt = np_sampled(A, Q, planes, **params)
        out, var = rendered_a.denoise_sampled_image(A, Q, planes, **params)
        assert_images_equal(out, want_out, f"frame c {params}: image")
        assert_images_equal(var, want_var, f"frame c {params}: variance")
    assert cnt["below_two"] == 2 and cnt["t_negative"] >= 1 and cnt["t_nan"] >= 1 and cnt["invalid"] == len(PLANTED_INVALID)
    for k in ("empty", "one", "negative"):
        assert var[PLANTED[k]][0] == 0.0, k
    thr = noise_threshold(A, Q)
    want_e, want_s = np_noise(A, Q, threshold=thr)
    e, s = rendered_a.noise_image(A, Q, threshold=thr)
    assert_images_equal(e, want_e, "frame c: error image")
    assert (s["pixels"], s["above"], F(s["max_error"])) == (want_s["pixels"], want_s["above"], F(want_s["max_error"]))
    want_e, want_s = np_noise(RULES_A, RULES_Q)
    assert np.isnan(want_e[1]) and want_e[4] < 0.0 and want_s["above"] == 3
    e, s = rendered_a.noise_image(RULES_A, RULES_Q)
    assert_errors_equal(e, want_e, "hand-made records")
    assert s == want_s
    for rows, want in ((slice(0, 3), {"pixels": 3, "above": 2, "max_error": float(want_e[0])}), (slice(4, 5), {"pixels": 1, "above": 0, "max_error": 0.0})):
        assert rendered_a.noise_image(RULES_A[rows], RULES_Q[rows])[1] == want, rows


def test_profiling_times_nest(product_scene):
    """Profiling mode: every timed kernel runs inside a render call's or a drain's bracket,
    so ms_total is at least the per-kernel times' sum; ms_accum is filled."""
    r = renderer(product_scene)
    try:
        r.set_profiling(True)
        r.render(16, 0)
        st = r.stats()
        parts = [st[k] for k in ("ms_sort", "ms_extend", "ms_shade", "ms_connect", "ms_regen", "ms_tail", "ms_accum")]
        assert st["ms_accum"] > 0.0 and st["ms_extend"] > 0.0, st
        assert st["ms_total"] >= sum(parts), (st["ms_total"], parts)
        A, Q, _, _ = frame_a()
        assert_words_equal(r.sample_squares(), Q, "squares in profiling mode")
    finally:
        r.close()


def test_row_shard_context_is_refused(rendered_shards):
    with pytest.raises(surf_amd.SurfError) as e:
        rendered_shards[1].denoise_sampled()
    assert e.value.code == SURF_ERR_INVALID and "surf_denoise_sampled_image" in str(e.value)


# ---- 3. the noise estimate ----------------------------------------------------------------------------

def test_noise_estimate_parity(rendered_a, rendered_shards):
    A, Q, _, _ = frame_a()
    thr = noise_threshold(A, Q)
    for kw in (dict(threshold=thr), {}, dict(threshold=thr, floor=0.5)):
        want_e, want_s = np_noise(A, Q, **kw)
        e, s = rendered_a.noise_estimate(**kw)
        assert_images_equal(e, want_e, f"noise_estimate {kw}: error image")
        assert s["pixels"] == W * H and s["above"] == want_s["above"], (s, want_s)
        assert F(s["max_error"]).view(np.uint32) == F(want_s["max_error"]).view(np.uint32), (s, want_s)
        none, s2 = rendered_a.noise_estimate(image=False, **kw)
        assert none is None and s2 == s
        ei, si = rendered_a.noise_image(A, Q, **kw)
        assert_images_equal(ei, want_e, f"noise_image {kw}: error image")
        assert si == s
        parts = [r.noise_estimate(**kw) for r in rendered_shards]
        assert_words_equal(surf_amd.assemble_shards(W, H, [np.repeat(p[0][..., None], 4, -1) for p in parts], SHARDS)[..., 0], want_e,
                           f"noise_estimate {kw}: the shards' error images")
        assert sum(p[1]["pixels"] for p in parts) == W * H and sum(p[1]["above"] for p in parts) == want_s["above"]
        assert F(max(p[1]["max_error"] for p in parts)).view(np.uint32) == F(want_s["max_error"]).view(np.uint32)
    want_s = np_noise(A, Q, threshold=thr)[1]
    assert 0 < want_s["above"] < want_s["pixels"]


# ---- 4. the device-to-device copies ----------------------------------------------------------------------

def test_copy_to_device(rendered_a):
    with open("/proc/self/maps") as maps:
        hip_path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    hip = C.CDLL(hip_path)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], \
        [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    dev = C.c_void_p()
    try:
        assert hip.hipMalloc(C.byref(dev), W * H * 16) == 0
        got = np.zeros((H, W, 4), np.float32)
        rendered_a.copy_sample_squares_to(dev.value)
        assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0       # hipMemcpyDeviceToHost
        assert_images_equal(got, rendered_a.sample_squares(), "copy_sample_squares_to")
        rendered_a.copy_denoise_sampled_to(dev.value, iterations=3)
        assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0
        assert_images_equal(got, rendered_a.denoise_sampled(iterations=3), "copy_denoise_sampled_to")
    finally:
        if dev.value:
            hip.hipFree(dev)


# ---- 5. the C++ API and the example ---------------------------------------------------------------------

def test_cpp_example_matches_python(product_scene, tmp_path):
    exe = os.path.join(surf_amd._PKG, "build", "render_denoised")
    word_rows = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    prefix = str(tmp_path / "sd")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "4", prefix], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = renderer(product_scene)
    try:
        r.render(1, 0, spp=4)                                       # the example's one frame of SPP samples
        want, plain = r.denoise_sampled(), r.denoise()
    finally:
        r.close()
    assert np.array_equal(word_rows(read_pfm(prefix + "_sampled.pfm")), word_rows(want[..., :3]))
    assert np.array_equal(word_rows(read_pfm(prefix + "_denoised.pfm")), word_rows(plain[..., :3]))      # as without the squares
    one = str(tmp_path / "one")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, "33", "9", "1", one], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert os.path.exists(one + "_denoised.pfm") and not os.path.exists(one + "_sampled.pfm")           # one sample has no variance
