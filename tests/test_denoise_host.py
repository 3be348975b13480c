"""The edge-avoiding a-trous denoiser (surf_denoise*, include/surf_hip.h) where
it needs no GPU: exported symbols and defaults, status codes, the CPU twin
(surf_denoise_image_host) against a numpy restatement, and the filter's gain
on the oracle's indoor scene.  CPU only.

Bar: bit-exact.  The expected image never comes from the code under test:
np_denoise below restates the header's arithmetic, every step an explicit
float32 numpy operation (single IEEE operations, no contraction) in the stated
order; its exp is glibc's expf, called through ctypes -- tests/test_libm.py
pins the library's gExpf to glibc on [-110, 0], and the filter clamps the
argument to [-100, 0].  Images are compared as uint32 words.

tests/test_gpu_denoise.py imports np_denoise and the frames from here.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import surf_amd
from test_gpu_aov import expected_planes

F = np.float32
SURF_ERR_INVALID = -1
W, H = 100, 37
H5 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
DEFAULTS = dict(iterations=5, sigma_color=1.0, sigma_normal=0.3, sigma_plane=0.1, demodulate=1)

_libm = C.CDLL("libm.so.6")
_libm.expf.argtypes, _libm.expf.restype = [C.c_float], C.c_float


def glibc_expf(x: np.ndarray) -> np.ndarray:
    """glibc's expf of every element (one libm call per distinct value)."""
    flat = np.ascontiguousarray(x, np.float32).ravel()
    uniq, inverse = np.unique(flat.view(np.uint32), return_inverse=True)
    vals = np.array([_libm.expf(float(v)) for v in uniq.view(np.float32)], np.float32)
    return vals[inverse].reshape(x.shape)


def np_denoise(acc, position, normal, albedo, iterations=5, sigma_color=1.0, sigma_normal=0.3, sigma_plane=0.1, demodulate=1):
    """The header's arithmetic on (H, W, 4) float32 planes; returns (H, W, 4)."""
    acc, position, normal, albedo = (np.asarray(a, np.float32) for a in (acc, position, normal, albedo))
    h, w = acc.shape[:2]
    with np.errstate(all="ignore"):
        valid = albedo[..., 3] != F(0.0)
        inv = np.where(acc[..., 3] > F(0.0), F(1.0) / acc[..., 3], F(0.0)).astype(np.float32)
        c = acc[..., :3] * inv[..., None]
        a3 = albedo[..., :3]
        den = np.where((valid & bool(demodulate))[..., None], np.where(a3 > F(0.01), a3, F(0.01)), F(1.0)).astype(np.float32)
        I = c / den
        N, P = normal[..., :3], position[..., :3]
        kn = F(1.0) / (F(sigma_normal) * F(sigma_normal))
        kp = F(1.0) / (F(sigma_plane) * F(sigma_plane))
        ys0, xs0 = np.arange(h), np.arange(w)
        for i in range(iterations):
            s = 1 << i
            sc = F(sigma_color) * np.ldexp(F(1.0), -i).astype(np.float32)
            kc = F(1.0) / (sc * sc)
            assert all(type(k) is np.float32 for k in (sc, kc, kn, kp))
            sum_w = np.zeros((h, w), np.float32)
            sm = np.zeros((h, w, 3), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ys, xs = ys0 + dy * s, xs0 + dx * s
                    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
                    yc, xc = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
                    take = lambda a: a[yc][:, xc]
                    use = inside & take(valid) & valid
                    Iq, Nq, Pq = take(I), take(N), take(P)
                    dC = Iq - I
                    dc = (dC[..., 0] * dC[..., 0] + dC[..., 1] * dC[..., 1]) + dC[..., 2] * dC[..., 2]
                    dN = Nq - N
                    dn = (dN[..., 0] * dN[..., 0] + dN[..., 1] * dN[..., 1]) + dN[..., 2] * dN[..., 2]
                    dP = Pq - P
                    pl = (dP[..., 0] * N[..., 0] + dP[..., 1] * N[..., 1]) + dP[..., 2] * N[..., 2]
                    dp = pl * pl
                    e = (dc * kc + dn * kn) + dp * kp
                    e = np.where(e < F(100.0), e, F(100.0)).astype(np.float32)
                    e = np.where(use, e, F(0.0))                      # skipped taps: any in-range argument, discarded below
                    wgt = (H5[dy + 2] * H5[dx + 2]) * glibc_expf(-e)
                    assert wgt.dtype == np.float32
                    sum_w = np.where(use, sum_w + wgt, sum_w)
                    sm = np.where(use[..., None], sm + wgt[..., None] * Iq, sm)
            I = np.where(valid[..., None], sm / sum_w[..., None], I).astype(np.float32)
        rgb = np.where(valid[..., None], I * den, c)
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = rgb
    assert rgb.dtype == np.float32
    return out


def synthetic_frame(w, h, seed):
    """(acc, planes): a seeded frame with two rectangular miss regions, one pixel
    without samples, albedo channels below the 0.01 clamp and unit normals."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    acc = np.empty((h, w, 4), np.float32)
    acc[..., :3] = rng.uniform(0.0, 8.0, (h, w, 3)).astype(np.float32)
    acc[..., 3] = F(4.0)
    acc[h // 2, w // 3] = (F(0.0), F(0.0), F(0.0), F(0.0))               # no sample at all
    base = np.where((xx < w / 2)[..., None], np.array([0, 0, 1], np.float32), np.array([0, 1, 0], np.float32))
    n = (base + rng.normal(0.0, 0.15, (h, w, 3))).astype(np.float32)
    n = n / np.sqrt((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])[..., None]
    normal = np.concatenate([n, np.zeros((h, w, 1), np.float32)], axis=-1).astype(np.float32)
    position = np.stack([xx * F(0.02), yy * F(0.02), rng.normal(0.0, 0.02, (h, w)).astype(np.float32),
                         np.ones((h, w), np.float32)], axis=-1).astype(np.float32)
    albedo = np.concatenate([rng.uniform(0.0, 1.0, (h, w, 3)), np.ones((h, w, 1))], axis=-1).astype(np.float32)
    albedo[: max(1, h // 3), :, 1] = rng.uniform(0.0, 0.01, (max(1, h // 3), w)).astype(np.float32)   # below the clamp
    albedo[0, 0, :3] = 0.0
    miss = np.zeros((h, w), bool)
    miss[h // 4: h // 4 + max(1, h // 5), w // 5: w // 5 + max(1, w // 4)] = True
    miss[h - max(1, h // 6):, w - max(1, w // 3):] = True
    albedo[miss] = (F(0.3), F(0.5), F(0.9), F(0.0))                      # the background, w = 0
    normal[miss] = 0.0
    position[miss] = (F(0.0), F(0.0), F(0.0), F(1e30))
    assert miss.any() and not miss.all() and (albedo[~miss][:, :3] < 0.01).any()
    return acc, {"position": position, "normal": normal, "albedo": albedo}


SYNTHETIC = {"b": (37, 23, 11), "c": (5, 3, 12), "tile": (33, 9, 13)}     # name -> (w, h, seed)


@pytest.fixture(scope="session")
def denoise_frames(oracle_scene):
    """name -> (acc, planes) of every frame the denoiser tests use (shared, read only):
    'a' the oracle's indoor scene at 100 x 37, 4 spp, with the oracle/numpy planes;
    'b' 37 x 23 synthetic; 'c' 5 x 3, smaller than the filter's footprint;
    'tile' 33 x 9, one 32 x 8 tile plus one pixel each way."""
    frames = {k: synthetic_frame(*v) for k, v in SYNTHETIC.items()}
    planes, _ = expected_planes(oracle_scene, oracle_scene.camera_ubo(W, H), W, range(H))
    acc = oracle_scene.render(W, H, 1, spp=4, max_segments=64)[0]
    frames["a"] = (acc, {k: planes[k] for k in ("position", "normal", "albedo")})
    for acc, pl in frames.values():
        acc.setflags(write=False)
        for a in pl.values():
            a.setflags(write=False)
    return frames


_expected = {}


def expected_image(frames, name, **params):
    """np_denoise of a shared frame, computed once per (frame, parameters)."""
    key = (name, tuple(sorted(params.items())))
    if key not in _expected:
        acc, pl = frames[name]
        img = np_denoise(acc, pl["position"], pl["normal"], pl["albedo"], **{**DEFAULTS, **params})
        img.setflags(write=False)
        _expected[key] = img
    return _expected[key]


def assert_images_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, f"{what}: {got.shape} {got.dtype}"
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first (row, x, channel) {bad[:4].tolist()}: "
                           f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


# ---- 1. symbols and defaults ---------------------------------------------------

def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in ("surf_denoise_default_params", "surf_denoise", "surf_denoise_copy_device", "surf_denoise_image",
                 "surf_denoise_image_host", "surf_debug_denoise_time"):
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4


def test_default_params():
    p = surf_amd.DenoiseParams()
    assert C.sizeof(p) == 32
    assert surf_amd.load().surf_denoise_default_params(C.byref(p)) == 0
    assert (p.iterations, p.demodulate) == (5, 1)
    assert (F(p.sigma_color), F(p.sigma_normal), F(p.sigma_plane)) == (F(1.0), F(0.3), F(0.1))
    q = surf_amd.denoise_params(iterations=3, sigma_plane=0.5)
    assert (q.iterations, F(q.sigma_color), F(q.sigma_plane), q.demodulate) == (3, F(1.0), F(0.5), 1)


# ---- 2. error paths --------------------------------------------------------------

def test_invalid_arguments_are_status_codes():
    lib = surf_amd.load()
    w, h = 4, 3
    buf = [np.ones((h, w, 4), np.float32) for _ in range(5)]
    ptr = [b.ctypes.data for b in buf]
    good = surf_amd.denoise_params()
    host = lib.surf_denoise_image_host
    assert host(w, h, *ptr[:4], C.byref(good), ptr[4]) == 0
    for k in range(5):                                                    # each plane and the output NULL
        args = list(ptr)
        args[k] = None
        assert host(w, h, *args[:4], C.byref(good), args[4]) == SURF_ERR_INVALID, k
    assert host(w, h, *ptr[:4], None, ptr[4]) == SURF_ERR_INVALID
    assert host(0, h, *ptr[:4], C.byref(good), ptr[4]) == SURF_ERR_INVALID
    assert host(w, 0, *ptr[:4], C.byref(good), ptr[4]) == SURF_ERR_INVALID
    for it in (0, 7, 0xFFFFFFFF):
        assert host(w, h, *ptr[:4], C.byref(surf_amd.denoise_params(iterations=it)), ptr[4]) == SURF_ERR_INVALID, it
    for it in (1, 6):
        assert host(w, h, *ptr[:4], C.byref(surf_amd.denoise_params(iterations=it)), ptr[4]) == 0, it
    for field in ("sigma_color", "sigma_normal", "sigma_plane"):
        for bad in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            p = surf_amd.denoise_params(**{field: bad})
            assert host(w, h, *ptr[:4], C.byref(p), ptr[4]) == SURF_ERR_INVALID, (field, bad)
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.denoise_image_host(buf[0], buf[1:4], iterations=9)
    assert e.value.code == SURF_ERR_INVALID and "iterations" in str(e.value)
    # a NULL context
    assert lib.surf_denoise_default_params(None) == SURF_ERR_INVALID
    assert lib.surf_denoise(None, C.byref(good), ptr[4]) == SURF_ERR_INVALID
    assert lib.surf_denoise_copy_device(None, C.byref(good), ptr[4]) == SURF_ERR_INVALID
    assert lib.surf_denoise_image(None, w, h, *ptr[:4], C.byref(good), ptr[4]) == SURF_ERR_INVALID
    ms = (C.c_float * 7)()
    assert lib.surf_debug_denoise_time(None, ms, 7) == SURF_ERR_INVALID


# ---- 3. the host twin equals numpy, bit for bit ----------------------------------

@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_host_twin_bitexact(denoise_frames, name, iterations, demodulate):
    acc, planes = denoise_frames[name]
    want = expected_image(denoise_frames, name, iterations=iterations, demodulate=demodulate)
    got = surf_amd.denoise_image_host(acc, planes, iterations=iterations, demodulate=demodulate)
    assert_images_equal(got, want, f"frame {name}, {iterations} iterations, demodulate {demodulate}")
    valid = planes["albedo"][..., 3] != 0
    assert (got[..., 3] == 1.0).all()
    # a miss passes through: radiance over sample count
    c = acc[..., :3] * (F(1.0) / F(4.0))
    assert np.array_equal(got[~valid][:, :3], c[~valid])
    # the filter did something where it may
    assert not np.array_equal(got[valid][:, :3], c[valid])


def test_frames_exercise_the_branches(denoise_frames):
    acc, planes = denoise_frames["b"]
    valid = planes["albedo"][..., 3] != 0
    assert (acc[..., 3] == 0).sum() == 1 and valid[acc[..., 3] == 0].all()
    n = planes["normal"][valid][:, :3].astype(np.float64)
    assert np.allclose((n * n).sum(-1), 1.0, atol=1e-6)
    assert (planes["albedo"][valid][:, :3] < 0.01).sum() > 10
    _, pa = denoise_frames["a"]
    miss = (pa["albedo"][..., 3] == 0).mean()
    assert 0.0 <= miss < 0.9


# ---- 4. quality --------------------------------------------------------------------

def test_denoised_is_closer_to_the_converged_image(oracle_scene, denoise_frames):
    """mean |denoised - ref| <= 0.6 * mean |noisy - ref| on the indoor scene at
    100 x 37, 4 spp against 1024 spp, default parameters (a numpy prototype
    with numpy's exp measured 0.43; the result is deterministic)."""
    osc = oracle_scene
    oracle.set_zero_cutoff(True)
    try:
        acc = osc.render(W, H, 1, spp=4, max_segments=64)[0]
        ref_acc = osc.render(W, H, 1, first_frame=1000, spp=1024, max_segments=64)[0]
    finally:
        oracle.set_zero_cutoff(False)
    _, planes = denoise_frames["a"]
    noisy = acc[..., :3] / acc[..., 3:4]
    ref = ref_acc[..., :3] / ref_acc[..., 3:4]
    got = surf_amd.denoise_image_host(acc, planes)[..., :3]
    err_noisy = float(np.abs(noisy.astype(np.float64) - ref).mean())
    err_got = float(np.abs(got.astype(np.float64) - ref).mean())
    print(f"mean abs error: noisy {err_noisy:.4f}, denoised {err_got:.4f}, ratio {err_got / err_noisy:.3f}")
    assert err_got <= 0.6 * err_noisy, (err_got, err_noisy)


# ---- 5. the example ----------------------------------------------------------------

def test_render_denoised_example_is_built():
    exe = os.path.join(os.path.dirname(surf_amd.LIB_PATH), "..", "build", "render_denoised")
    assert os.path.isfile(exe) and os.access(exe, os.X_OK)
