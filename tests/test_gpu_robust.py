"""The sample buckets on the device (surf_set_sample_buckets: the planes
k_accumulate_buckets keeps) and the robust estimate (surf_robust_*), against the
oracle's per-sample radiance and the numpy restatements of tests/test_robust_host.py.

Bar: bit-exact, planes and images compared as uint32 words.  The expected values
never come from the code under test: the buckets are summed in float32 numpy from
the oracle's spp-1 frames by the header's rule, the estimates are np_robust's.

Every frame is 100 x 37: 3,700 pixels, no multiple of the wave nor of the
256-thread block, so the guards and the partial last wave are exercised.
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
from test_robust_host import BUCKET_COUNTS, PLANTED, assert_robust_equal, np_buckets, np_halves, np_robust, planted
from test_sampled_host import H, W, np_squares, oracle_samples

pytestmark = pytest.mark.gpu
F = np.float32
SURF_ERR_INVALID = -1
COUNTERS = ("samples", "n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")
FRAMES = 19                                       # uneven counts: with M = 16 three buckets hold two samples, thirteen one


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


def assert_words_equal(got, want, what):
    assert_images_equal(np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32), what)


_want = {}


def expected(M, frames=FRAMES):
    """(A, B) of the oracle's first `frames` samples, computed once per M."""
    if (M, frames) not in _want:
        _want[M, frames] = np_buckets(oracle_samples(frames)[0], M)
    return _want[M, frames]


_off = {}


def buckets_off(scene, squares, batch, frames=FRAMES, spp=1):
    """(accumulator, squares, counters) of a context with buckets off, rendered once per setting."""
    key = (squares, batch, frames, spp)
    if key not in _off:
        r = renderer(scene, 0, squares, frame_batch=batch)
        try:
            r.render(frames, 0, spp=spp)
            st = r.stats()
            _off[key] = (r.accumulator(), r.sample_squares() if squares else None, [st[k] for k in COUNTERS])
        finally:
            r.close()
    return _off[key]


# ---- 1. the bucket planes ----------------------------------------------------------------------------

@pytest.mark.parametrize("squares", [False, True], ids=["plain", "squares"])
@pytest.mark.parametrize("batch", [1, 24], ids=["batch1", "batch24"])
@pytest.mark.parametrize("M", [4, 16])
def test_buckets_bitexact(product_scene, M, batch, squares):
    """19 spp-1 frames; a frame batch of 1 accumulates pass by pass (the read-modify-write path), one of 24 lets a
    launch take M passes or more from a count that is a multiple of M (the grouped path)."""
    A, B = expected(M)
    counts = sorted(set(B[:, 0, 0, 3].tolist()))
    assert counts == ([4.0, 5.0] if M == 4 else [1.0, 2.0]) and (B[:, :, :, 3].sum(0) == FRAMES).all()
    off_acc, off_sq, off_counters = buckets_off(product_scene, squares, batch)
    r = renderer(product_scene, M, squares, frame_batch=batch)
    try:
        assert r.sample_bucket_count() == M
        r.render(FRAMES, 0)
        got, acc, st = r.sample_buckets(), r.accumulator(), r.stats()
        assert got.shape == (M, H, W, 4)
        assert_words_equal(got, B, f"buckets, M = {M}")
        assert_words_equal(acc, A, "accumulator against the oracle's samples")
        assert_words_equal(acc, off_acc, "accumulator, buckets on against off")
        if squares:
            assert_words_equal(r.sample_squares(), off_sq, "squares, buckets on against off")
            assert_words_equal(off_sq, np_squares(oracle_samples(FRAMES)[0])[1], "squares against the oracle's samples")
        assert [st[k] for k in COUNTERS] == off_counters
        print(f"M = {M}, frame batch {batch}: window {st['frame_window']}")
    finally:
        r.close()


def test_long_stream_groups(product_scene):
    """48 frames with M = 16 under the default frame batch (a window of 256 passes): launches that take several
    whole groups of 16 passes, then a tail; how many passes a launch takes is the host's batching, which nothing here pins."""
    A, B = expected(16, 48)
    r = renderer(product_scene, 16, True)
    try:
        r.render(48, 0)
        assert_words_equal(r.sample_buckets(), B, "buckets, 48 frames, M = 16")
        assert_words_equal(r.accumulator(), A, "accumulator, 48 frames")
        assert_words_equal(r.sample_squares(), np_squares(oracle_samples(48)[0])[1], "squares, 48 frames")
        even, odd = surf_amd.bucket_halves(r.sample_buckets())
        assert_words_equal(even, np_halves(B)[0], "even half")
        assert_words_equal(odd, np_halves(B)[1], "odd half")
    finally:
        r.close()


@pytest.mark.parametrize("squares", [False, True], ids=["plain", "squares"])
def test_multi_sample_frames(product_scene, squares):
    """5 frames of 4 samples: the buckets are per pass.  The per-sample radiance of a chained frame is not the
    oracle's to give: the counts, the partition and the unchanged outputs."""
    off_acc, off_sq, off_counters = buckets_off(product_scene, squares, None, 5, 4)
    r = renderer(product_scene, 8, squares)
    try:
        r.render(5, 0, spp=4)
        B, acc, st = r.sample_buckets(), r.accumulator(), r.stats()
        assert_words_equal(acc, off_acc, "accumulator of 5 frames of 4 samples, buckets on against off")
        if squares:
            assert_words_equal(r.sample_squares(), off_sq, "squares of 5 frames of 4 samples, buckets on against off")
        assert [st[k] for k in COUNTERS] == off_counters
        for j in range(8):
            assert (B[j, :, :, 3] == (3.0 if j < 4 else 2.0)).all(), j
        total = np.zeros_like(acc)
        for j in range(8):
            total = total + B[j]
        assert (total[..., 3] == 20.0).all() and np.allclose(total, acc, rtol=1e-4, atol=1e-6)     # the same 20 samples, another order
    finally:
        r.close()


def checkerboard():
    yy, xx = np.mgrid[0:H, 0:W]
    return ((yy + xx) & 1).astype(np.uint8)


def test_masked_stream(product_scene):
    """8 frames, a checkerboard mask, 5 frames, an all-ones mask, 3 frames: the bucket of each sample follows the
    pixel's own count (8 .. 12 on the active squares, then 8 .. 10 on the others), inactive records stay untouched."""
    samples = oracle_samples(16)[0]
    mask = checkerboard()
    M = 4
    A1, B1 = np_buckets(samples[:8], M)
    A2, B2 = np_buckets(samples[8:13], M, A1, B1, mask)
    A3, B3 = np_buckets(samples[13:16], M, A2, B2)
    assert sorted(set(A3[..., 3].ravel().tolist())) == [11.0, 16.0]
    r = renderer(product_scene, M, True)
    try:
        r.render(8, 0)
        r.set_pixel_mask(mask)
        r.render(5, 8)
        got2, acc2 = r.sample_buckets(), r.accumulator()
        assert_words_equal(got2, B2, "buckets after the masked frames")
        assert_words_equal(acc2, A2, "accumulator after the masked frames")
        assert_words_equal(got2[:, mask == 0], B1[:, mask == 0], "the inactive pixels' bucket records")
        r.set_pixel_mask(np.ones((H, W), np.uint8))
        r.render(3, 13)
        assert_words_equal(r.sample_buckets(), B3, "buckets after the all-ones mask")
        assert_words_equal(r.accumulator(), A3, "accumulator after the all-ones mask")
    finally:
        r.close()


def test_drop_in_loop(product_scene):
    A, B = np_buckets(oracle_samples(12)[0], 8)
    r = renderer(product_scene, 8)
    try:
        for j in range(12):
            r.render(1, j)
        assert_words_equal(r.sample_buckets(), B, "buckets, twelve one-frame calls")
        assert_words_equal(r.accumulator(), A, "accumulator, twelve one-frame calls")
    finally:
        r.close()


def test_row_shards(product_scene):
    """Two interleaved row shards, assembled plane by plane, equal the full frame's planes; the estimate works per shard."""
    M = 4
    A, B = expected(M)
    specs = [ShardSpec(k, 2, 2) for k in range(2)]
    rs = [renderer(product_scene, M, shard=s) for s in specs]
    try:
        for r in rs:
            r.render(FRAMES, 0)
        parts = [r.sample_buckets() for r in rs]
        assert all(p.shape == (M, len(r.rows), W, 4) for p, r in zip(parts, rs))
        full = np.stack([surf_amd.assemble_shards(W, H, [p[j] for p in parts], specs) for j in range(M)])
        assert_words_equal(full, B, "bucket planes assembled from two row shards")
        want = np_robust(A, B)
        est = [r.robust() for r in rs]
        assert_words_equal(surf_amd.assemble_shards(W, H, [e[0] for e in est], specs), want[0], "the estimate, per shard")
        assert sum(e[2]["trimmed"] for e in est) == want[2]["trimmed"] and sum(e[2]["pixels"] for e in est) == W * H
    finally:
        for r in rs:
            r.close()


def test_lifecycle(product_scene):
    r = surf_amd.Renderer(product_scene, W, H)
    dev_err = lambda f, *a, **k: pytest.raises(surf_amd.SurfError, f, *a, **k).value.code
    try:
        assert r.sample_bucket_count() == 0
        for call in (r.sample_buckets, r.robust):                                 # off: every context form refuses
            assert dev_err(call) == SURF_ERR_INVALID
        for m in (1, 3, 6, 32):
            assert dev_err(r.set_sample_buckets, m) == SURF_ERR_INVALID
        r.render(2, 0)
        assert dev_err(r.set_sample_buckets, 4) == SURF_ERR_INVALID                # samples present: their buckets are lost
        r.clear_accumulator()
        r.set_sample_buckets(4)
        assert not r.sample_buckets().any()
        r.render(3, 0)
        samples = oracle_samples(3)[0]
        assert_words_equal(r.sample_buckets(), np_buckets(samples, 4)[1], "buckets after clear + enable")
        assert dev_err(r.set_sample_buckets, 0) == SURF_ERR_INVALID
        assert dev_err(r.set_sample_buckets, 8) == SURF_ERR_INVALID
        r.clear_accumulator()
        assert not r.sample_buckets().any() and not r.accumulator().any()
        r.set_sample_buckets(16)                                                   # a larger M after a clear
        r.render(3, 0)
        assert_words_equal(r.sample_buckets(), np_buckets(samples, 16)[1], "buckets, M = 16 after M = 4")
        r.clear_accumulator()
        r.set_sample_buckets(2)                                                    # a smaller one keeps the allocation
        assert r.sample_bucket_count() == 2 and r.sample_buckets().shape == (2, H, W, 4) and not r.sample_buckets().any()
        r.render(3, 0)
        assert_words_equal(r.sample_buckets(), np_buckets(samples, 2)[1], "buckets, M = 2 after M = 16")
        r.clear_accumulator()
        r.set_sample_buckets(0)
        r.render(3, 0)
        assert dev_err(r.sample_buckets) == SURF_ERR_INVALID
        assert_words_equal(r.accumulator(), np_buckets(samples, 2)[0], "accumulator with the buckets switched off again")
    finally:
        r.close()


# ---- 2. the robust estimate ------------------------------------------------------------------------------

@pytest.mark.parametrize("M", BUCKET_COUNTS)
def test_robust_on_rendered_buckets(product_scene, M):
    A, B = expected(M, 48)
    want = np_robust(A, B)
    assert (want[2]["trimmed"] > 0) == (M > 2)
    r = renderer(product_scene, M)
    try:
        r.render(48, 0)
        got = r.robust()
        assert_robust_equal(got, want, f"surf_robust_accumulator, M = {M}")
        assert_robust_equal(r.robust_image(r.accumulator(), r.sample_buckets()), want, f"surf_robust_image on the read-back planes, M = {M}")
        assert_robust_equal(surf_amd.robust_image_host(A, B), want, f"the host twin, M = {M}")
        out, trim, s = r.robust(trim_scale=2.0, image=False)
        want2 = np_robust(A, B, 2.0)
        assert trim is None and s == want2[2]
        assert_words_equal(out, want2[0], f"trim_scale 2 without a trim image, M = {M}")
        assert r.debug_robust_time() > 0.0
    finally:
        r.close()


@pytest.mark.parametrize("M", BUCKET_COUNTS)
def test_robust_on_planted_inputs(product_scene, M):
    """Needs no buckets on the context: the image form uploads its planes."""
    A, B, at = planted(M)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        for ts in (1.0, 4.0, 0.0):
            want = np_robust(A, B, ts)
            assert_robust_equal(r.robust_image(A, B, trim_scale=ts), want, f"planted, M = {M}, trim_scale {ts}")
            assert_robust_equal(surf_amd.robust_image_host(A, B, trim_scale=ts), want, f"planted on the host, M = {M}, trim_scale {ts}")
        k = at["outlier"]
        assert_robust_equal(r.robust_image(A[k:k + 1], B[:, k:k + 1]), np_robust(A[k:k + 1], B[:, k:k + 1]), f"one pixel, M = {M}")
        big_a, big_b = np.tile(A, (37, 1)), np.tile(B, (1, 37, 1))                   # 296 pixels: more than one block, a partial last wave
        assert_robust_equal(r.robust_image(big_a, big_b), np_robust(big_a, big_b), f"planted x 37, M = {M}")
        lib = surf_amd.load()
        out, trim, s = np.zeros_like(A), np.zeros(len(PLANTED), np.uint8), surf_amd.RobustSummary()
        p = surf_amd.robust_params()
        args = lambda npx=len(PLANTED), m=M, a=A.ctypes.data, b=B.ctypes.data, pp=C.byref(p), o=out.ctypes.data: \
            (r.handle, npx, m, a, b, pp, o, trim.ctypes.data, C.byref(s))
        assert lib.surf_robust_image(*args()) == 0
        for bad in (args(npx=0), args(m=3), args(m=0), args(a=None), args(b=None), args(pp=None), args(o=None),
                    args(pp=C.byref(surf_amd.robust_params(float("nan")))), args(pp=C.byref(surf_amd.robust_params(-1.0)))):
            assert lib.surf_robust_image(*bad) == SURF_ERR_INVALID
    finally:
        r.close()


def test_cpp_example_matches_python(product_scene, tmp_path):
    """render_denoised ... 0 8: one frame of 32 samples with 8 buckets; the robust accumulator feeds both filters."""
    exe = os.path.join(surf_amd._PKG, "build", "render_denoised")
    words = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    prefix = str(tmp_path / "rb")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "32", prefix, "0", "8"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = renderer(product_scene, 8, True)
    try:
        r.render(1, 0, spp=32)
        acc, trim, s = r.robust()
        planes = r.aov()
        plain = r.denoise_image(acc, planes)
        guided = r.denoise_sampled_image(acc, r.sample_squares(), planes)[0]
        noisy = r.accumulator()
    finally:
        r.close()
    assert s["trimmed"] > 0
    with np.errstate(all="ignore"):
        mean = acc[..., :3] * np.where(acc[..., 3:] > 0, F(1.0) / acc[..., 3:], F(0.0))
        noisy = noisy[..., :3] * (F(1.0) / noisy[..., 3:])
    assert np.array_equal(words(read_pfm(prefix + "_robust.pfm")), words(mean))
    assert np.array_equal(words(read_pfm(prefix + "_noisy.pfm")), words(noisy))
    assert np.array_equal(words(read_pfm(prefix + "_denoised.pfm")), words(plain[..., :3]))
    assert np.array_equal(words(read_pfm(prefix + "_sampled.pfm")), words(guided[..., :3]))
    assert not os.path.exists(prefix + "_adaptive.pfm")
    bad = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "32", prefix, "0", "5"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "ROBUST_M" in bad.stderr


def test_copy_to_device(product_scene):
    with open("/proc/self/maps") as maps:
        hip_path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    hip = C.CDLL(hip_path)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], \
        [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    M = 8
    r = renderer(product_scene, M)
    dev = C.c_void_p()
    try:
        r.render(FRAMES, 0)
        assert hip.hipMalloc(C.byref(dev), M * W * H * 16) == 0
        got = np.zeros((M, H, W, 4), np.float32)
        r.copy_sample_buckets_to(dev.value)
        assert hip.hipMemcpy(got.ctypes.data, dev, M * W * H * 16, 2) == 0          # hipMemcpyDeviceToHost
        assert_images_equal(got, r.sample_buckets(), "copy_sample_buckets_to")
        assert_images_equal(got, expected(M)[1], "copy_sample_buckets_to against the oracle's samples")
        r.copy_robust_to(dev.value)
        assert hip.hipMemcpy(got[0].ctypes.data, dev, W * H * 16, 2) == 0
        assert_images_equal(got[0], r.robust()[0], "copy_robust_to")
        assert_images_equal(got[0], np_robust(*expected(M))[0], "copy_robust_to against np_robust")
    finally:
        if dev.value:
            hip.hipFree(dev)
        r.close()
