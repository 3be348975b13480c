"""The dual-buffer non-local-means filter (surf_denoise_nlm*, include/surf_hip.h)
where it needs no GPU: exported symbols and defaults, status codes, the CPU twin
against a numpy restatement, the branches the inputs reach, and the filter's error
against the sample-variance-guided filter's at 64 samples per pixel on the oracle's
indoor scene.  CPU only.

Bar: bit-exact, images compared as uint32 words.  The expected images never come
from the code under test: np_nlm below restates the header's rules, every step an
explicit float32 numpy operation in the stated order, vectorised per search offset;
exp is glibc's expf.  The halves are summed here in numpy from the oracle's
per-sample radiance.

tests/test_gpu_nlm.py imports the restatement, the frames and the parameters from here.
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from test_denoise_host import assert_images_equal, glibc_expf
from test_robust_host import np_buckets, np_halves, reference
from test_sampled_host import H, W, oracle_samples, quality

F = np.float32
SURF_ERR_INVALID = -1
DEFAULTS = dict(search_radius=5, patch_radius=2, k=0.45, alpha=1.0, eps=1e-10)
RADII = ((1, 0), (3, 1), (5, 2), (10, 3))


def np_nlm(half0, half1, **params):
    """The header's arithmetic on two (H, W, 4) half accumulators.  Returns (out, err, counts of the branches taken)."""
    sp = {**DEFAULTS, **params}
    assert set(params) <= set(DEFAULTS)
    H0, H1 = np.asarray(half0, np.float32), np.asarray(half1, np.float32)
    h, w = H0.shape[:2]
    r, f = int(sp["search_radius"]), int(sp["patch_radius"])
    kk = F(sp["k"]) * F(sp["k"])
    alpha, eps, cnt = F(sp["alpha"]), F(sp["eps"]), F(3 * (2 * f + 1) * (2 * f + 1))
    assert kk.dtype == np.float32
    ys, xs = np.arange(h), np.arange(w)
    take = lambda a, yy, xx: a[np.clip(yy, 0, h - 1)][:, np.clip(xx, 0, w - 1)]          # clampF
    count = {k: 0 for k in ("outside", "invalid_tap", "clamp_100", "clamp_0", "between", "vm_b", "vm_a", "invalid_pixel")}
    with np.errstate(all="ignore"):
        # ---- prepare
        n0, n1 = H0[..., 3], H1[..., 3]
        ok = (n0 > F(0.0)) & (n1 > F(0.0))
        q0, q1 = H0[..., :3] / n0[..., None], H1[..., :3] / n1[..., None]
        valid = ok & np.isfinite(q0).all(-1) & np.isfinite(q1).all(-1)
        c = [np.where(valid[..., None], q, F(0.0)).astype(np.float32) for q in (q0, q1)]
        dc = c[0] - c[1]
        v = F(0.5) * (dc * dc)
        V = np.zeros((h, w, 3), np.float32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                V = V + take(v, ys + dy, xs + dx)
        V = V / F(9.0)
        assert v.dtype == V.dtype == np.float32
        count["invalid_pixel"] = int((~valid).sum())
        # ---- the patch distances of every offset, both halves: E[offset, g] is the clamped e
        ye, xe = np.arange(-f, h + f), np.arange(-f, w + f)                              # the texels s', up to f outside the frame
        Ca, Va = [take(c[g], ye, xe) for g in (0, 1)], take(V, ye, xe)
        offsets = [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]
        E = np.zeros((len(offsets), 2, h, w), np.float32)
        use = np.zeros((len(offsets), h, w), bool)
        for oi, (dx, dy) in enumerate(offsets):
            inside = ((ys + dy >= 0) & (ys + dy < h))[:, None] & ((xs + dx >= 0) & (xs + dx < w))[None, :]
            vq = take(valid, ys + dy, xs + dx)
            use[oi] = valid & inside & vq
            count["outside"] += int((valid & ~inside).sum())
            count["invalid_tap"] += int((valid & inside & ~vq).sum())
            if dx == 0 and dy == 0:
                continue
            Vb = take(V, ye + dy, xe + dx)
            lower = Vb < Va
            vm = np.where(lower, Vb, Va)
            count["vm_b"] += int(lower.sum())
            count["vm_a"] += int((~lower).sum())
            for g in (0, 1):
                dl = Ca[g] - take(c[g], ye + dy, xe + dx)
                num = dl * dl - alpha * (Va + vm)
                den = eps + kk * (Va + Vb)
                d = num / den
                dsum = (d[..., 0] + d[..., 1]) + d[..., 2]
                assert dsum.dtype == np.float32
                S = np.zeros((h, w), np.float32)
                for j in range(2 * f + 1):                                               # rows first ...
                    R = np.zeros((h, w), np.float32)
                    for i in range(2 * f + 1):
                        R = R + dsum[j:j + h, i:i + w]
                    S = S + R                                                            # ... then the column of row sums
                D = S / cnt
                below = D < F(100.0)
                e = np.where(below, D, F(100.0)).astype(np.float32)                      # a NaN becomes 100
                above = e > F(0.0)
                e = np.where(above, e, F(0.0)).astype(np.float32)
                count["clamp_100"] += int((use[oi] & ~below).sum())
                count["clamp_0"] += int((use[oi] & below & ~above).sum())
                count["between"] += int((use[oi] & below & above).sum())
                E[oi, g] = e
        Wt = glibc_expf(-E)
        assert Wt.dtype == np.float32
        # ---- the weighted sums: half h takes its weights from half 1 - h
        sum_w = [np.zeros((h, w), np.float32) for _ in (0, 1)]
        sums = [np.zeros((h, w, 3), np.float32) for _ in (0, 1)]
        for oi, (dx, dy) in enumerate(offsets):
            centre = dx == 0 and dy == 0
            for hh in (0, 1):
                wgt = np.ones((h, w), np.float32) if centre else Wt[oi, 1 - hh]
                cq = take(c[hh], ys + dy, xs + dx)
                sum_w[hh] = np.where(use[oi], sum_w[hh] + wgt, sum_w[hh])
                sums[hh] = np.where(use[oi][..., None], sums[hh] + wgt[..., None] * cq, sums[hh])
        o0, o1 = sums[0] / sum_w[0][..., None], sums[1] / sum_w[1][..., None]
        rgb = ((o0 * n0[..., None]) + (o1 * n1[..., None])) / (n0 + n1)[..., None]
        do = o0 - o1
        er = F(0.25) * (do * do)
        n = n0 + n1
        inv = np.where(n > F(0.0), F(1.0) / n, F(0.0)).astype(np.float32)
        plain = (H0[..., :3] + H1[..., :3]) * inv[..., None]
        rgb = np.where(valid[..., None], rgb, plain)
        er = np.where(valid[..., None], er, F(0.0))
    assert rgb.dtype == er.dtype == np.float32
    out, err = np.ones((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    out[..., :3] = rgb
    err[..., :3] = er
    return out, err, count


# ---- the inputs ----------------------------------------------------------------------------------

_cache = {}


def halves(count, w=W, h=H, M=2):
    """The two halves of the oracle's first `count` samples at w x h, through M buckets; computed once, read only."""
    key = (count, w, h, M)
    if key not in _cache:
        pair = np_halves(np_buckets(oracle_samples(count, w, h)[0], M)[1])
        for a in pair:
            a.setflags(write=False)
        _cache[key] = tuple(pair)
    return _cache[key]


PLANTED = {"empty": (1, 3), "nan": (4, 8), "inf": (7, 12), "huge": (2, 16)}
BLOCK = (slice(2, 7), slice(20, 29))              # rows 2..6, columns 20..28: H0 * n1 == H1 * n0 exactly


def planted():
    """The 33 x 9 frame of 6 samples with: a pixel whose half 1 is empty; a NaN channel; an inf channel; a huge (1e30)
    channel, whose neighbours' v overflows; a block of identical half means, inside which V = 0 and the distance is
    divided by eps."""
    h0, h1 = (a.copy() for a in halves(6, 33, 9, 4))
    h1[PLANTED["empty"]] = 0.0
    h0[PLANTED["nan"]][1] = np.nan
    h0[PLANTED["inf"]][0] = np.inf
    h0[PLANTED["huge"]][2] = 1e30
    h0[BLOCK] = (0.75, 1.5, 0.375, 3.0)
    h1[BLOCK] = (0.75, 1.5, 0.375, 3.0)
    return h0, h1


def frame(name):
    if name == "a":                 # 100 x 37, 16 samples
        return halves(16)
    if name == "b6":                # 33 x 9, 6 samples through 4 buckets: no multiple of any tile, lower than the search window at r = 5
        return halves(6, 33, 9, 4)
    if name == "b5":                # 33 x 9, 5 samples: the halves hold 3 and 2
        return halves(5, 33, 9)
    if name == "strip":             # 70 x 3
        return halves(4, 70, 3)
    if name == "one":               # 1 x 1
        return halves(4, 1, 1)
    if name == "planted":
        return planted()
    if name == "identical":         # the same half twice: V = 0 everywhere
        return halves(6, 33, 9, 4)[0], halves(6, 33, 9, 4)[0]
    raise KeyError(name)


FRAMES = ("a", "b6", "b5", "strip", "one", "planted", "identical")
CASES = [(name, rf) for name in FRAMES for rf in RADII]
_want = {}


def expected(name, rf):
    """np_nlm of a frame at (r, f), computed once (the GPU tests ask for the same ones)."""
    if (name, rf) not in _want:
        _want[name, rf] = np_nlm(*frame(name), search_radius=rf[0], patch_radius=rf[1])
    return _want[name, rf]


# ---- 1. symbols and defaults -----------------------------------------------------------------------

NEW_SYMBOLS = ("surf_nlm_default_params", "surf_denoise_nlm", "surf_denoise_nlm_copy_device", "surf_denoise_nlm_image",
               "surf_denoise_nlm_image_host", "surf_debug_nlm_time")


def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("NlmParams", "nlm_params", "denoise_nlm_image_host"):
        assert hasattr(surf_amd, name), name
    for name in ("denoise_nlm", "denoise_nlm_image", "copy_denoise_nlm_to", "debug_nlm_time"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_params():
    p = surf_amd.NlmParams()
    assert C.sizeof(p) == 24
    p.search_radius, p.k, p._pad = 9, 7.0, 3
    assert surf_amd.load().surf_nlm_default_params(C.byref(p)) == 0
    assert (p.search_radius, p.patch_radius, p._pad) == (5, 2, 0)
    assert (F(p.k), F(p.alpha), F(p.eps)) == (F(0.45), F(1.0), F(1e-10))
    q = surf_amd.nlm_params(search_radius=3, eps=1e-6)
    assert (q.search_radius, q.patch_radius, F(q.k), F(q.eps)) == (3, 2, F(0.45), F(1e-6))
    with pytest.raises(TypeError):
        surf_amd.nlm_params(sigma=1.0)
    assert {k: getattr(p, k) for k in ("search_radius", "patch_radius")} == {k: DEFAULTS[k] for k in ("search_radius", "patch_radius")}


# ---- 2. status codes ---------------------------------------------------------------------------------

def test_invalid_arguments_are_status_codes():
    lib = surf_amd.load()
    h0, h1 = frame("b5")
    h, w = h0.shape[:2]
    out, err = np.zeros_like(h0), np.zeros_like(h0)
    good = surf_amd.nlm_params(search_radius=1, patch_radius=0)
    gb = C.byref(good)
    host = lib.surf_denoise_nlm_image_host
    a, b, o, e = h0.ctypes.data, h1.ctypes.data, out.ctypes.data, err.ctypes.data
    assert host(w, h, a, b, gb, o, e) == 0
    assert host(w, h, a, b, gb, o, None) == 0                                   # the error image is optional
    for bad in ((w, h, None, b, gb, o, e), (w, h, a, None, gb, o, e), (w, h, a, b, None, o, e), (w, h, a, b, gb, None, e),
                (0, h, a, b, gb, o, e), (w, 0, a, b, gb, o, e)):
        assert host(*bad) == SURF_ERR_INVALID, bad
    nan, inf = float("nan"), float("inf")
    for field, values in (("search_radius", (0, 11)), ("patch_radius", (4,)), ("k", (0.0, nan, inf, -1.0)), ("alpha", (-1.0, -1e-30, nan, inf)),
                          ("eps", (0.0, -1.0, nan, inf))):
        for val in values:
            p = surf_amd.nlm_params(**{"search_radius": 1, "patch_radius": 0, field: val})
            assert host(w, h, a, b, C.byref(p), o, e) == SURF_ERR_INVALID, (field, val)
    for field, values in (("search_radius", (1, 10)), ("patch_radius", (0, 3)), ("k", (1e-3, 10.0)), ("alpha", (0.0, 4.0)), ("eps", (1e-30, 1.0))):
        for val in values:
            p = surf_amd.nlm_params(**{"search_radius": 1, "patch_radius": 0, field: val})
            assert host(w, h, a, b, C.byref(p), o, e) == 0, (field, val)
    with pytest.raises(surf_amd.SurfError) as ex:
        surf_amd.denoise_nlm_image_host(h0, h1, search_radius=11)
    assert ex.value.code == SURF_ERR_INVALID and "search_radius" in str(ex.value)
    with pytest.raises(ValueError):
        surf_amd.denoise_nlm_image_host(h0, h1[:, :5])
    # a NULL context
    ms = (C.c_float * 3)()
    assert lib.surf_nlm_default_params(None) == SURF_ERR_INVALID
    assert lib.surf_denoise_nlm(None, gb, o, e) == SURF_ERR_INVALID
    assert lib.surf_denoise_nlm_copy_device(None, gb, o, e) == SURF_ERR_INVALID
    assert lib.surf_denoise_nlm_image(None, w, h, a, b, gb, o, e) == SURF_ERR_INVALID
    assert lib.surf_debug_nlm_time(None, ms, 3) == SURF_ERR_INVALID


# ---- 3. the host twin equals numpy, bit for bit ----------------------------------------------------

def assert_nlm_equal(got, want, what):
    assert_images_equal(got[0], want[0], f"{what}: image")
    assert_images_equal(got[1], want[1], f"{what}: err")


@pytest.mark.parametrize("name,rf", CASES, ids=[f"{n}-r{r}f{f}" for n, (r, f) in CASES])
def test_host_twin_bitexact(name, rf):
    h0, h1 = frame(name)
    want = expected(name, rf)
    print(f"{name} {h0.shape[1]} x {h0.shape[0]}, r {rf[0]}, f {rf[1]}: {want[2]}")
    assert_nlm_equal(surf_amd.denoise_nlm_image_host(h0, h1, search_radius=rf[0], patch_radius=rf[1]), want, f"{name}, r {rf[0]}, f {rf[1]}")


def test_other_scalars_bitexact():
    """k, alpha and eps away from their defaults, alpha = 0 (no variance cancellation) among them."""
    h0, h1 = frame("b5")
    for kw in (dict(k=1.0, alpha=0.0), dict(k=0.2, alpha=2.0, eps=1e-4)):
        sp = dict(search_radius=3, patch_radius=1, **kw)
        assert_nlm_equal(surf_amd.denoise_nlm_image_host(h0, h1, **sp), np_nlm(h0, h1, **sp), str(kw))


def test_frames_are_what_they_claim():
    assert frame("a")[0].shape == (37, 100, 4) and (frame("a")[0][..., 3] == 8).all() and (frame("a")[1][..., 3] == 8).all()
    assert frame("b6")[0].shape == (9, 33, 4) and (frame("b6")[0][..., 3] == 3).all() and (frame("b6")[1][..., 3] == 3).all()
    assert (frame("b5")[0][..., 3] == 3).all() and (frame("b5")[1][..., 3] == 2).all()
    assert frame("strip")[0].shape == (3, 70, 4) and frame("one")[0].shape == (1, 1, 4)
    h0, h1 = frame("planted")
    assert h1[PLANTED["empty"]][3] == 0 and np.isnan(h0[PLANTED["nan"]]).sum() == 1 and np.isinf(h0[PLANTED["inf"]]).sum() == 1
    assert np.array_equal(h0[BLOCK] * h1[BLOCK][..., 3:], h1[BLOCK] * h0[BLOCK][..., 3:])


# ---- 4. the inputs reach every branch ----------------------------------------------------------------

def test_inputs_reach_every_branch():
    total = {}
    for name, rf in CASES:
        for k, v in expected(name, rf)[2].items():
            total[k] = total.get(k, 0) + v
    print(total)
    for k in ("outside", "invalid_tap", "clamp_100", "clamp_0", "between", "vm_b", "vm_a", "invalid_pixel"):
        assert total[k] > 0, k
    # what each planted record is there for, at the defaults
    out, err, cnt = expected("planted", (5, 2))
    assert cnt["invalid_pixel"] == 3 and cnt["invalid_tap"] > 0 and cnt["clamp_100"] > 0 and cnt["clamp_0"] > 0
    for k in ("empty", "nan", "inf"):
        assert not err[PLANTED[k]].any(), k
    h0, h1 = frame("planted")
    e = PLANTED["empty"]
    assert np.array_equal(out[e][:3], (h0[e][:3] + h1[e][:3]) * (F(1.0) / F(3.0))) and out[e][3] == 1           # the plain mean of the half that has samples
    assert np.isnan(out[PLANTED["nan"]][1]) and np.isinf(out[PLANTED["inf"]][0])
    assert np.isfinite(out[PLANTED["huge"]]).all()                                                     # the huge pixel is valid ...
    with np.errstate(all="ignore"):
        c0, c1 = h0[..., :3] / h0[..., 3:], h1[..., :3] / h1[..., 3:]
        y, x = PLANTED["huge"]
        assert np.isinf(F(0.5) * ((c0[y, x, 2] - c1[y, x, 2]) * (c0[y, x, 2] - c1[y, x, 2])))              # ... and its v overflows
    # identical halves: the two filtered halves agree, the error estimate is 0
    assert not expected("identical", (5, 2))[1].any()


# ---- 5. quality ------------------------------------------------------------------------------------

RATIO_64 = 1.04      # np_nlm measures 0.9004 against np_sampled; x 1.15, rounded up to two decimals


def test_nlm_against_the_sample_variance_guided_filter_at_64_samples():
    """The oracle's indoor scene at 100 x 37, spp-1 frames from frame 0 through two buckets, default
    parameters, mean absolute error over all pixels against the oracle's 2048-spp render of the same view
    (first_frame 100000), set up as test_sampled_host.quality sets it up: np_nlm against np_sampled, the
    sample-variance-guided filter, of the same samples -- both restatements, never the library.  The
    asserted ratio is np_nlm's measured one x 1.15, rounded up to two decimals (test_sampled_host's
    RATIO_64 convention; the margin is for parameter retuning, the result is deterministic); that the
    filter's error is below the noisy mean's is a condition.  N = 16 is printed, not asserted.  np_nlm
    measures (MEASUREMENTS "Non-local means"), noisy / fixed-sigma / sample-variance-guided / non-local means:
    N = 16  0.03749 / 0.01453 / 0.01407 / 0.01388, ratio 0.9864;
    N = 64  0.02164 / 0.01309 / 0.01154 / 0.01039, ratio 0.9004, asserted <= 1.04.
    Both ratios are below 1: without a feature plane the filter is ahead of the best guided one here."""
    res = quality((16, 64), 2048)
    ref = reference()
    mae = lambda img: float(np.abs(img[..., :3].astype(np.float64) - ref).mean())
    got = {}
    for n in (16, 64):
        noisy, fixed, guided = res[n][:3]
        h0, h1 = halves(n)
        out = np_nlm(h0, h1)[0]
        got[n] = (noisy, guided, mae(out), out, h0, h1)
        print(f"N = {n}: noisy {noisy:.5f}, fixed-sigma {fixed:.5f}, sample-variance-guided {guided:.5f}, non-local means {got[n][2]:.5f}, "
              f"ratio to sample-variance-guided {got[n][2] / guided:.4f}")
    noisy, guided, nlm, want, h0, h1 = got[64]
    assert_images_equal(surf_amd.denoise_nlm_image_host(h0, h1)[0], want, "the host twin at 64 samples")
    assert nlm < noisy, (nlm, noisy)
    assert nlm / guided <= RATIO_64, (nlm / guided, nlm, guided)
