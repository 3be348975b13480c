"""The per-sample second moments' two readers (surf_denoise_sampled*, surf_noise_*,
include/surf_hip.h) where they need no GPU: exported symbols and defaults, status
codes, the CPU twins against numpy restatements, the branches the frames reach,
and the sample-variance-guided filter's gain over the fixed-sigma filter at 64
samples per pixel on the oracle's indoor scene.  CPU only.

Bar: bit-exact, images compared as uint32 words.  The expected images never come
from the code under test: np_sampled and np_noise below restate the header's
arithmetic, every step an explicit float32 numpy operation in the stated order
(step C as tests/test_svgf_host.py's np_svgf states it); exp is glibc's expf.
The squares are summed here in numpy from the oracle's per-sample radiance.

tests/test_gpu_sampled.py imports the restatements and the frames from here.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import surf_amd
from test_denoise_host import H5, assert_images_equal, glibc_expf, np_denoise
from test_gpu_aov import UNSET, expected_planes
from test_svgf_host import G3, lum

F = np.float32
W, H = 100, 37
SURF_ERR_INVALID = -1
DEFAULTS = dict(iterations=5, sigma_lum=4.0, sigma_normal=0.3, sigma_plane=0.1, demodulate=1, variance_eps=1e-10)
NO_ESTIMATE = F(1e30)


def np_squares(samples):
    """(A, Q) of per-sample (H, W, 4) radiance planes (w = 1 each), summed in f32 in sample order."""
    A = np.zeros_like(samples[0])
    Q = np.zeros_like(samples[0])
    for r in samples:
        r = np.asarray(r, np.float32)
        A = A + r
        l = lum(r)
        Q = Q + np.stack([r[..., 0] * r[..., 0], r[..., 1] * r[..., 1], r[..., 2] * r[..., 2], l * l], -1)
    assert A.dtype == np.float32 and Q.dtype == np.float32
    return A, Q


def np_sampled(acc, squares, planes, **params):
    """The header's arithmetic: level 0 from A and Q, then step C of the variance-guided
    filter.  planes: a dict with 'position', 'normal', 'albedo'.  Returns (out, variance, counts)."""
    sp = {**DEFAULTS, **params}
    assert set(params) <= set(DEFAULTS)
    A, Q, P4, N4, alb = (np.asarray(a, np.float32) for a in (acc, squares, planes["position"], planes["normal"], planes["albedo"]))
    h, w = A.shape[:2]
    cnt = {}
    with np.errstate(all="ignore"):
        valid = alb[..., 3] != F(0.0)
        n = A[..., 3]
        inv = np.where(n > F(0.0), F(1.0) / n, F(0.0)).astype(np.float32)
        c = A[..., :3] * inv[..., None]
        a3 = alb[..., :3]
        den = np.where((valid & bool(sp["demodulate"]))[..., None], np.where(a3 > F(0.01), a3, F(0.01)), F(1.0)).astype(np.float32)
        # ---- level 0
        est = valid & (n >= F(2.0))
        m = Q[..., :3] * inv[..., None]
        t = m - c * c
        pos = t > F(0.0)
        s = np.sqrt(np.where(pos, t, F(0.0)).astype(np.float32)) / den
        sd = lum(s)
        v = np.where(est, (sd * sd) / (n - F(1.0)), F(0.0)).astype(np.float32)
        cnt["invalid"] = int((~valid).sum())
        cnt["below_two"] = int((valid & ~(n >= F(2.0))).sum())
        cnt["empty"] = int((valid & (n == F(0.0))).sum())
        cnt["one_sample"] = int((valid & (n == F(1.0))).sum())
        cnt["estimated"] = int(est.sum())
        cnt["t_nan"] = int((est[..., None] & np.isnan(t)).sum())
        cnt["t_negative"] = int((est[..., None] & (t < F(0.0))).sum())
        I = np.concatenate([c / den, v[..., None]], -1).astype(np.float32)
        var = np.zeros((h, w, 4), np.float32)
        var[..., 0] = v
        # ---- step C (np_svgf's, restated)
        Nn, Pp = N4[..., :3], P4[..., :3]
        kn = F(1.0) / (F(sp["sigma_normal"]) * F(sp["sigma_normal"]))
        kp = F(1.0) / (F(sp["sigma_plane"]) * F(sp["sigma_plane"]))
        sl, eps = F(sp["sigma_lum"]), F(sp["variance_eps"])
        ys0, xs0 = np.arange(h), np.arange(w)

        def guides(ys, xs):
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            yc, xc = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
            take = lambda a: a[yc][:, xc]
            dN = take(Nn) - Nn
            dn = (dN[..., 0] * dN[..., 0] + dN[..., 1] * dN[..., 1]) + dN[..., 2] * dN[..., 2]
            dP = take(Pp) - Pp
            pl = (dP[..., 0] * Nn[..., 0] + dP[..., 1] * Nn[..., 1]) + dP[..., 2] * Nn[..., 2]
            return inside & take(valid) & valid, take, dn, pl * pl

        for i in range(sp["iterations"]):
            step = 1 << i
            gs, gw = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    use, take, _, _ = guides(ys0 + dy, xs0 + dx)
                    g = G3[dy + 1][dx + 1]
                    gs = np.where(use, gs + g * take(I)[..., 3], gs)
                    gw = np.where(use, gw + g, gw)
            gv = gs / gw
            kl = F(1.0) / (sl * np.sqrt(gv) + eps)
            assert kl.dtype == np.float32
            lp = lum(I)
            sum_w, sum_v, sm = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    use, take, dn, dp = guides(ys0 + dy * step, xs0 + dx * step)
                    Iq = take(I)
                    dl = np.abs(lum(Iq) - lp)
                    e = (dl * kl + dn * kn) + dp * kp
                    e = np.where(e < F(100.0), e, F(100.0)).astype(np.float32)
                    e = np.where(use, e, F(0.0))                          # skipped taps: any in-range argument, discarded
                    wgt = (H5[dy + 2] * H5[dx + 2]) * glibc_expf(-e)
                    assert wgt.dtype == np.float32
                    sum_w = np.where(use, sum_w + wgt, sum_w)
                    sm = np.where(use[..., None], sm + wgt[..., None] * Iq[..., :3], sm)
                    sum_v = np.where(use, sum_v + (wgt * wgt) * Iq[..., 3], sum_v)
            nxt = np.concatenate([sm / sum_w[..., None], (sum_v / (sum_w * sum_w))[..., None]], -1)
            I = np.where(valid[..., None], nxt, I).astype(np.float32)
        var[..., 1] = np.where(valid, I[..., 3], F(0.0))
        rgb = np.where(valid[..., None], I[..., :3] * den, I[..., :3])
    assert rgb.dtype == np.float32
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = rgb
    return out, var, cnt


def np_noise(acc, squares, threshold=0.05, floor=0.01):
    """The header's noise estimate: (error image, summary dict)."""
    A, Q = np.asarray(acc, np.float32), np.asarray(squares, np.float32)
    with np.errstate(all="ignore"):
        n = A[..., 3]
        inv = F(1.0) / n
        lb = lum(A[..., :3] * inv[..., None])
        t = Q[..., 3] * inv - lb * lb
        t = np.where(t > F(0.0), t, F(0.0)).astype(np.float32)
        e = np.sqrt(t / (n - F(1.0))) / (lb + F(floor))
        e = np.where(n >= F(2.0), e, NO_ESTIMATE).astype(np.float32)
        above = int((~(e <= F(threshold))).sum())
        good = e[e > F(0.0)]                                              # a NaN and a negative e leave the maximum, which starts at 0, alone
    return e, {"pixels": int(e.size), "above": above, "max_error": float(good.max()) if good.size else 0.0}


# ---- the frames -----------------------------------------------------------------------

_cache = {}


def oracle_samples(count, w=W, h=H):
    """The oracle's first `count` spp-1 frames of the bundled scene's default view, (h, w, 4)
    each, and the view's feature planes with the oracle's hit mask; computed once, read only."""
    key = (w, h)
    if key not in _cache or len(_cache[key][0]) < count:
        osc = oracle.OracleScene()
        oracle.set_zero_cutoff(True)
        try:
            ubo = osc.camera_ubo(w, h)
            samples = [osc.render(w, h, 1, first_frame=j)[0] for j in range(count)]
            planes, info = expected_planes(osc, ubo, w, range(h))
        finally:
            oracle.set_zero_cutoff(False)
            osc.close()
        for a in samples + list(planes.values()):
            a.setflags(write=False)
        _cache[key] = (samples, planes, info["hit"].reshape(h, w))
    samples, planes, hit = _cache[key]
    return samples[:count], planes, hit


def frame_a():
    """100 x 37, 16 samples."""
    samples, planes, hit = oracle_samples(16)
    if "a" not in _cache:
        _cache["a"] = np_squares(samples)
    return (*_cache["a"], planes, hit)


def frame_b():
    """33 x 9, 5 samples: no multiple of the tile either way."""
    samples, planes, hit = oracle_samples(5, 33, 9)
    if "b" not in _cache:
        _cache["b"] = np_squares(samples)
    return (*_cache["b"], planes, hit)


PLANTED = {"empty": (2, 3), "one": (2, 4), "negative": (3, 5), "nan": (3, 6)}
PLANTED_INVALID = [(5, 10), (5, 11), (0, 0)]          # the bundled view is a closed room: no pixel misses on its own


def frame_c():
    """Frame B with planted records at valid pixels: no sample, one sample, squares too
    small for the mean (t < 0), NaN squares; and invalid pixels (albedo.w = 0, as on a miss)."""
    A, Q, planes, hit = frame_b()
    A, Q, hit = A.copy(), Q.copy(), hit.copy()
    alb = planes["albedo"].copy()
    for p in PLANTED_INVALID:
        alb[p] = (0.25, 0.5, 0.75, 0.0)
        hit[p] = False
    planes = {**planes, "albedo": alb}
    for y, x in PLANTED.values():
        assert hit[y, x], (y, x)
    A[PLANTED["empty"]] = 0.0
    Q[PLANTED["empty"]] = 0.0
    A[PLANTED["one"]] = (0.25, 0.5, 0.125, 1.0)
    Q[PLANTED["one"]] = (0.0625, 0.25, 0.015625, lum(np.array([0.25, 0.5, 0.125], np.float32)) ** 2)
    Q[PLANTED["negative"]] = Q[PLANTED["negative"]] * F(0.001)
    Q[PLANTED["nan"]][1] = np.nan
    Q[PLANTED["nan"]][3] = np.nan
    return A, Q, planes, hit


FRAMES = {"a": frame_a, "b": frame_b, "c": frame_c}


def noise_threshold(A, Q):
    """The median of the frame's estimated errors: pixels on both sides (numpy only)."""
    e, _ = np_noise(A, Q)
    return float(np.median(e[e < NO_ESTIMATE]))


# ---- 1. symbols and defaults ---------------------------------------------------------------

NEW_SYMBOLS = ("surf_set_sample_squares", "surf_read_sample_squares", "surf_copy_sample_squares_device", "surf_denoise_sampled",
               "surf_denoise_sampled_copy_device", "surf_denoise_sampled_image", "surf_denoise_sampled_image_host", "surf_debug_sampled_time",
               "surf_noise_default_params", "surf_noise_estimate", "surf_noise_image", "surf_noise_image_host")


def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("NoiseParams", "NoiseSummary", "noise_params", "denoise_sampled_image_host", "noise_image_host"):
        assert hasattr(surf_amd, name), name
    for name in ("set_sample_squares", "sample_squares", "copy_sample_squares_to", "denoise_sampled", "denoise_sampled_image",
                 "copy_denoise_sampled_to", "debug_sampled_time", "noise_estimate", "noise_image"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_params():
    p = surf_amd.NoiseParams()
    assert C.sizeof(p) == 8 and C.sizeof(surf_amd.NoiseSummary) == 24
    assert surf_amd.load().surf_noise_default_params(C.byref(p)) == 0
    assert (F(p.threshold), F(p.floor)) == (F(0.05), F(0.01))
    q = surf_amd.noise_params(floor=0.5)
    assert (F(q.threshold), F(q.floor)) == (F(0.05), F(0.5))
    A, Q, planes, _ = frame_b()
    with pytest.raises(TypeError):
        surf_amd.denoise_sampled_image_host(A, Q, planes, spatial_below=4)
    with pytest.raises(TypeError):
        surf_amd.denoise_sampled_image_host(A, Q, planes, sigma_color=1.0)


# ---- 2. status codes -------------------------------------------------------------------------

def test_invalid_arguments_are_status_codes():
    lib = surf_amd.load()
    A, Q, planes, _ = frame_b()
    w, h, a = surf_amd._sampled_planes(A, Q, planes)
    ptr = [x.ctypes.data for x in a]
    out, var = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    good = surf_amd.svgf_params()
    gb = C.byref(good)
    host = lib.surf_denoise_sampled_image_host
    assert host(w, h, *ptr, gb, out.ctypes.data, var.ctypes.data) == 0
    for k in range(5):                                                                   # each plane NULL
        args = list(ptr)
        args[k] = None
        assert host(w, h, *args, gb, out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID, k
    assert host(w, h, *ptr, None, out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID
    assert host(w, h, *ptr, gb, None, var.ctypes.data) == SURF_ERR_INVALID
    assert host(w, h, *ptr, gb, out.ctypes.data, None) == SURF_ERR_INVALID
    assert host(0, h, *ptr, gb, out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID
    assert host(w, 0, *ptr, gb, out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID
    bad = {"iterations": (0, 7, 0xFFFFFFFF)}
    for field in ("sigma_lum", "sigma_normal", "sigma_plane", "variance_eps"):
        bad[field] = (0.0, -1.0, float("nan"), float("inf"), float("-inf"))
    for field, values in bad.items():
        for v in values:
            p = surf_amd.svgf_params(**{field: v})
            assert host(w, h, *ptr, C.byref(p), out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID, (field, v)
    for field, values in {"iterations": (1, 6), "spatial_below": (0, 1, 0xFFFFFFFF)}.items():     # spatial_below is ignored
        for v in values:
            p = surf_amd.svgf_params(**{field: v})
            assert host(w, h, *ptr, C.byref(p), out.ctypes.data, var.ctypes.data) == 0, (field, v)
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.denoise_sampled_image_host(A, Q, planes, iterations=0)
    assert e.value.code == SURF_ERR_INVALID and "iterations" in str(e.value)
    # the noise estimate
    npx = w * h
    err = np.zeros(npx, np.float32)
    s = surf_amd.NoiseSummary()
    np_ = surf_amd.noise_params()
    nhost = lib.surf_noise_image_host
    assert nhost(npx, ptr[0], ptr[1], C.byref(np_), err.ctypes.data, C.byref(s)) == 0
    assert nhost(npx, ptr[0], ptr[1], C.byref(np_), None, C.byref(s)) == 0                    # the image is optional
    assert nhost(0, ptr[0], ptr[1], C.byref(np_), err.ctypes.data, C.byref(s)) == SURF_ERR_INVALID
    assert nhost(npx, None, ptr[1], C.byref(np_), err.ctypes.data, C.byref(s)) == SURF_ERR_INVALID
    assert nhost(npx, ptr[0], None, C.byref(np_), err.ctypes.data, C.byref(s)) == SURF_ERR_INVALID
    assert nhost(npx, ptr[0], ptr[1], None, err.ctypes.data, C.byref(s)) == SURF_ERR_INVALID
    assert nhost(npx, ptr[0], ptr[1], C.byref(np_), err.ctypes.data, None) == SURF_ERR_INVALID
    for field in ("threshold", "floor"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            p = surf_amd.noise_params(**{field: v})
            assert nhost(npx, ptr[0], ptr[1], C.byref(p), err.ctypes.data, C.byref(s)) == SURF_ERR_INVALID, (field, v)
    # a NULL context
    assert lib.surf_noise_default_params(None) == SURF_ERR_INVALID
    assert lib.surf_set_sample_squares(None, 1) == SURF_ERR_INVALID
    assert lib.surf_read_sample_squares(None, out.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_copy_sample_squares_device(None, out.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_denoise_sampled(None, gb, out.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_denoise_sampled_copy_device(None, gb, out.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_denoise_sampled_image(None, w, h, *ptr, gb, out.ctypes.data, var.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_noise_estimate(None, C.byref(np_), err.ctypes.data, C.byref(s)) == SURF_ERR_INVALID
    assert lib.surf_noise_image(None, npx, ptr[0], ptr[1], C.byref(np_), err.ctypes.data, C.byref(s)) == SURF_ERR_INVALID
    ms = (C.c_float * 7)()
    assert lib.surf_debug_sampled_time(None, ms, 7) == SURF_ERR_INVALID


# ---- 3. the host twins equal numpy, bit for bit ----------------------------------------------

HOST_CASES = [("a", {}), ("b", {}), ("c", {}), ("b", dict(iterations=1)), ("c", dict(iterations=6, demodulate=0)),
              ("a", dict(iterations=2, sigma_lum=1.0, demodulate=0))]


@pytest.mark.parametrize("name,params", HOST_CASES, ids=[f"{c[0]}-{'-'.join(f'{k}{v}' for k, v in c[1].items())}" for c in HOST_CASES])
def test_host_twin_bitexact(name, params):
    A, Q, planes, _ = FRAMES[name]()
    want_out, want_var, _ = np_sampled(A, Q, planes, **params)
    out, var = surf_amd.denoise_sampled_image_host(A, Q, planes, **params)
    assert_images_equal(out, want_out, f"case {name} {params}: image")
    assert_images_equal(var, want_var, f"case {name} {params}: variance")
    assert (out[..., 3] == 1.0).all() and (var[..., 2:] == 0.0).all()


def test_inputs_reach_every_branch():
    A, Q, planes, hit = frame_a()
    cnt = np_sampled(A, Q, planes, iterations=1)[2]
    print("frame a", cnt)
    assert cnt["invalid"] == int((~hit).sum())                    # frame A has misses exactly where the oracle says so
    assert cnt["invalid"] == int((planes["id"][..., 0] == UNSET).sum())
    assert cnt["estimated"] == int(hit.sum()) and cnt["below_two"] == 0
    A, Q, planes, hit = frame_c()
    cnt = np_sampled(A, Q, planes, iterations=1)[2]
    print("frame c", cnt)
    assert cnt["empty"] == 1 and cnt["one_sample"] == 1 and cnt["below_two"] == 2
    assert cnt["t_negative"] >= 1 and cnt["t_nan"] >= 1
    assert cnt["invalid"] == int((~hit).sum()) == len(PLANTED_INVALID)
    _, var, _ = np_sampled(A, Q, planes)
    got = surf_amd.denoise_sampled_image_host(A, Q, planes)[1]    # ... and the twin takes the same branches there
    for k in ("empty", "one", "negative"):
        assert var[PLANTED[k]][0] == 0.0 and got[PLANTED[k]][0] == 0.0, k      # no estimate, or every t_k clamped to 0
    assert got[PLANTED["nan"]][0] == var[PLANTED["nan"]][0] > 0.0             # the NaN t_y is 0, the other channels count
    for p in PLANTED_INVALID:
        assert got[p][0] == 0.0 and got[p][1] == 0.0, p


def test_fewer_than_two_samples_everywhere_is_valid():
    """n = 1 everywhere: v = 0, kl = 1 / variance_eps, and the filter all but returns its input."""
    samples, planes, hit = oracle_samples(1, 33, 9)
    A, Q = np_squares(samples)
    out, var = surf_amd.denoise_sampled_image_host(A, Q, planes)
    want_out, want_var, cnt = np_sampled(A, Q, planes)
    assert cnt["estimated"] == 0
    assert_images_equal(out, want_out, "n = 1: image")
    assert_images_equal(var, want_var, "n = 1: variance")
    assert (var[..., 0] == 0.0).all()
    lit = hit & (lum(A) > F(1e-3))
    assert lit.sum() > 50 and np.abs(out[..., :3][lit] - A[..., :3][lit]).max() <= 1e-4 * np.abs(A[..., :3]).max()


# ---- 4. the noise estimate ---------------------------------------------------------------------

@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_noise_host_twin_exact(name):
    A, Q, _, _ = FRAMES[name]()
    thr = noise_threshold(A, Q)
    want_e, want_s = np_noise(A, Q, threshold=thr)
    if name == "a":
        assert 0 < want_s["above"] < want_s["pixels"], want_s       # pixels on both sides of the threshold
    if name == "c":
        assert want_e[PLANTED["empty"]] == NO_ESTIMATE and want_e[PLANTED["one"]] == NO_ESTIMATE
        assert want_e[PLANTED["nan"]] == 0.0                        # a NaN t becomes 0
    e, s = surf_amd.noise_image_host(A, Q, threshold=thr)
    assert_images_equal(e, want_e, f"frame {name}: error image")
    assert s["pixels"] == want_s["pixels"] == A.shape[0] * A.shape[1] and s["above"] == want_s["above"], (s, want_s)
    assert F(s["max_error"]).view(np.uint32) == F(want_s["max_error"]).view(np.uint32), (s, want_s)
    e0, s0 = surf_amd.noise_image_host(A, Q)                         # the defaults
    w0 = np_noise(A, Q)
    assert_images_equal(e0, w0[0], f"frame {name}: error image, default parameters")
    assert (s0["above"], F(s0["max_error"])) == (w0[1]["above"], F(w0[1]["max_error"]))


# hand-made records: an ordinary pixel, a NaN mean, a black pixel, one sample, a negative mean luminance
RULES_A = np.array([[4.0, 4.0, 4.0, 4.0], [np.nan, 1.0, 1.0, 4.0], [0.0, 0.0, 0.0, 3.0], [2.0, 2.0, 2.0, 1.0], [-2.0, -2.0, -2.0, 2.0]], np.float32)
RULES_Q = np.array([[8.0, 8.0, 8.0, 8.0], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0], [4.0, 4.0, 4.0, 4.0], [4.0, 4.0, 4.0, 4.0]], np.float32)


def assert_errors_equal(got, want, what):
    """Words equal, except that a NaN need only be a NaN: the header prescribes no payload."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaNs at {np.isnan(got)}, want {np.isnan(want)}"
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), f"{what}: {got} != {want}"


def test_noise_summary_rules():
    """A NaN error counts as above the threshold and leaves the maximum alone, as a negative
    one does, which does not count; the maximum starts at 0."""
    A, Q = RULES_A, RULES_Q
    want_e, want_s = np_noise(A, Q)
    assert np.isnan(want_e[1]) and want_e[2] == 0.0 and want_e[3] == NO_ESTIMATE and 0.0 < want_e[0] < 1.0 and want_e[4] < 0.0
    assert want_s == {"pixels": 5, "above": 3, "max_error": float(NO_ESTIMATE)}
    e, s = surf_amd.noise_image_host(A, Q)
    assert_errors_equal(e, want_e, "hand-made records")
    assert s == want_s
    e, s = surf_amd.noise_image_host(A[4:], Q[4:])
    assert s == {"pixels": 1, "above": 0, "max_error": 0.0}
    e, s = surf_amd.noise_image_host(A[:3], Q[:3])
    assert s == {"pixels": 3, "above": 2, "max_error": float(want_e[0])}


# ---- 5. quality ----------------------------------------------------------------------------------

RATIO_64 = 1.02      # np_sampled measures 0.8815; x 1.15, rounded up -- so the bound that binds is "strictly below 1"


def quality(counts, ref_spp, ref_first=100000):
    """{N: (noisy, fixed-sigma, sample-variance-guided) mean absolute errors} against the
    oracle's ref_spp render of the same view; default parameters everywhere."""
    samples, planes, _ = oracle_samples(max(counts))
    osc = oracle.OracleScene()
    oracle.set_zero_cutoff(True)
    try:
        osc.camera_ubo(W, H)
        ref_acc = osc.render(W, H, 1, first_frame=ref_first, spp=ref_spp, max_segments=64)[0]
    finally:
        oracle.set_zero_cutoff(False)
        osc.close()
    ref = ref_acc[..., :3].astype(np.float64) / ref_acc[..., 3:4]
    err = lambda img: float(np.abs(img[..., :3].astype(np.float64) - ref).mean())
    res = {}
    for n in counts:
        A, Q = np_squares(samples[:n])
        fixed = np_denoise(A, planes["position"], planes["normal"], planes["albedo"])
        guided = np_sampled(A, Q, planes)[0]
        res[n] = (err(A / A[..., 3:4]), err(fixed), err(guided), A, Q, planes, guided)
    return res


def test_sample_variance_guided_filter_gains_at_64_samples():
    """The oracle's indoor scene at 100 x 37, 64 spp-1 frames from frame 0, default
    parameters, mean absolute error over all pixels against the oracle's 2048-spp
    render of the same view (first_frame 100000): np_sampled against np_denoise, the
    fixed-sigma filter, of the same accumulator.  The asserted ratio is np_sampled's
    measured one x 1.15, rounded up to two decimals; N = 4 and N = 16 are printed,
    not asserted (MEASUREMENTS "Sample-variance-guided filter").  np_sampled measures
    (the result is deterministic), noisy / fixed-sigma / sample-variance-guided:
    N = 4   0.0611 / 0.0189 / 0.0191, ratio 1.0101;
    N = 16  0.0375 / 0.0145 / 0.0141, ratio 0.9683;
    N = 64  0.0216 / 0.0131 / 0.0115, ratio 0.8815, asserted <= 1.02 and < 1."""
    res = quality((4, 16, 64), 2048)
    for n, (noisy, fixed, guided, *_rest) in res.items():
        print(f"N = {n}: noisy {noisy:.4f}, fixed-sigma {fixed:.4f}, sample-variance-guided {guided:.4f}, ratio {guided / fixed:.4f}")
    noisy, fixed, guided, A, Q, planes, want = res[64]
    out, _ = surf_amd.denoise_sampled_image_host(A, Q, planes)
    assert_images_equal(out, want, "the host twin at 64 samples")
    ratio = guided / fixed
    assert ratio < 1.0 and ratio <= RATIO_64, (ratio, res[64][:3])
    assert guided < noisy
