"""The first-order feature regression filter (surf_denoise_regress*, include/surf_hip.h)
where it needs no GPU: exported symbols and defaults, status codes, the CPU twin against
a numpy restatement, the branches the inputs reach, the identity with the non-local-means
filter on constant planes, and the filter's error against non-local means' on the oracle's
indoor scene.  CPU only.

Bar: bit-exact, images compared as uint32 words.  The expected images never come from the
code under test: np_regress below restates the header's rules, every step an explicit
float32 numpy operation in the stated order, vectorised per search offset, the elimination
written out entry by entry; exp is glibc's expf.  The halves are summed in numpy from the
oracle's per-sample radiance, the planes are the oracle's or test_denoise_host's synthetic ones.

tests/test_gpu_regress.py imports the restatement, the frames and the parameters from here.
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from test_denoise_host import assert_images_equal, glibc_expf, synthetic_frame
from test_nlm_host import RADII, frame, halves, np_nlm
from test_robust_host import reference
from test_sampled_host import H, W, oracle_samples, quality

F = np.float32
SURF_ERR_INVALID = -1
DEFAULTS = dict(search_radius=5, patch_radius=2, k=0.7, alpha=1.0, eps=1e-10, ridge=0.1)
BRANCHES = ("outside", "invalid_tap", "miss_tap", "nonfinite_tap", "miss_centre", "invalid_pixel", "fallback_pivot", "fallback_beta",
            "solved", "clamp_100", "clamp_0", "between")
DIM = 8


def np_regress(half0, half1, planes, **params):
    """The header's arithmetic on two (H, W, 4) half accumulators and the three feature planes.
    Returns (out, err, counts of the branches taken)."""
    sp = {**DEFAULTS, **params}
    assert set(params) <= set(DEFAULTS)
    if isinstance(planes, dict):
        planes = [planes[k] for k in ("position", "normal", "albedo")]
    H0, H1 = np.asarray(half0, np.float32), np.asarray(half1, np.float32)
    pos, nrm, alb = (np.asarray(a, np.float32) for a in planes)
    h, w = H0.shape[:2]
    r, f = int(sp["search_radius"]), int(sp["patch_radius"])
    kk = F(sp["k"]) * F(sp["k"])
    alpha, eps, ridge, cnt = F(sp["alpha"]), F(sp["eps"]), F(sp["ridge"]), F(3 * (2 * f + 1) * (2 * f + 1))
    assert kk.dtype == np.float32
    ys, xs = np.arange(h), np.arange(w)
    take = lambda a, yy, xx: a[np.clip(yy, 0, h - 1)][:, np.clip(xx, 0, w - 1)]          # clampF
    finite = lambda a: (a - a) == F(0.0)
    count = {k: 0 for k in BRANCHES}
    with np.errstate(all="ignore"):
        # ---- prepare: surf_denoise_nlm's
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
        # ---- the feature records
        feat = [nrm[..., 0], nrm[..., 1], nrm[..., 2], alb[..., 0], alb[..., 1], alb[..., 2]]
        z = pos[..., 3]
        hit = alb[..., 3] != F(0.0)
        count["invalid_pixel"] = int((~valid).sum())
        count["miss_centre"] = int((valid & ~hit).sum())
        # ---- the sums, offset by offset
        ye, xe = np.arange(-f, h + f), np.arange(-f, w + f)                              # the texels s', up to f outside the frame
        Ca, Va = [take(c[g], ye, xe) for g in (0, 1)], take(V, ye, xe)
        one = np.ones((h, w), np.float32)
        A = [[[np.zeros((h, w), np.float32) for _ in range(DIM)] for _ in range(DIM)] for _ in (0, 1)]       # A[half][i][j], i <= j
        b = [[[np.zeros((h, w), np.float32) for _ in range(3)] for _ in range(DIM)] for _ in (0, 1)]         # b[half][i][channel]
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                centre = dx == 0 and dy == 0
                inside = ((ys + dy >= 0) & (ys + dy < h))[:, None] & ((xs + dx >= 0) & (xs + dx < w))[None, :]
                vq = take(valid, ys + dy, xs + dx)
                hq = take(hit, ys + dy, xs + dx)
                phi = [take(a, ys + dy, xs + dx) - a for a in feat]
                phi.append((take(z, ys + dy, xs + dx) - z) / z)
                fin = np.ones((h, w), bool)
                for p in phi:
                    fin = fin & finite(p)
                phi.append(one)
                assert all(p.dtype == np.float32 for p in phi)
                use1 = valid & hit & inside & vq & hq & fin                                # a hit centre's accepted taps
                use0 = valid & ~hit & inside & vq                                          # a miss centre's
                use = use1 | use0
                count["outside"] += int((valid & ~inside).sum())
                count["invalid_tap"] += int((valid & inside & ~vq).sum())
                count["miss_tap"] += int((valid & hit & inside & vq & ~hq).sum())
                count["nonfinite_tap"] += int((valid & hit & inside & vq & hq & ~fin).sum())
                wgt = [one, one]                                                           # wgt[g]: from the distance in half g
                if not centre:
                    Vb = take(V, ye + dy, xe + dx)
                    vm = np.where(Vb < Va, Vb, Va)
                    wgt = []
                    for g in (0, 1):
                        dl = Ca[g] - take(c[g], ye + dy, xe + dx)
                        num = dl * dl - alpha * (Va + vm)
                        den = eps + kk * (Va + Vb)
                        d = num / den
                        dsum = (d[..., 0] + d[..., 1]) + d[..., 2]
                        S = np.zeros((h, w), np.float32)
                        for j in range(2 * f + 1):                                       # rows first ...
                            R = np.zeros((h, w), np.float32)
                            for i in range(2 * f + 1):
                                R = R + dsum[j:j + h, i:i + w]
                            S = S + R                                                    # ... then the column of row sums
                        D = S / cnt
                        below = D < F(100.0)
                        e = np.where(below, D, F(100.0)).astype(np.float32)              # a NaN becomes 100
                        above = e > F(0.0)
                        e = np.where(above, e, F(0.0)).astype(np.float32)
                        count["clamp_100"] += int((use & ~below).sum())
                        count["clamp_0"] += int((use & below & ~above).sum())
                        count["between"] += int((use & below & above).sum())
                        wgt.append(glibc_expf(-e))
                cq = [take(c[hh], ys + dy, xs + dx) for hh in (0, 1)]
                for i in range(DIM):
                    for j in range(i, DIM):
                        pp = phi[i] * phi[j]
                        on = use if i == DIM - 1 else use1                                 # order zero: the last row alone
                        for hh in (0, 1):
                            A[hh][i][j] = np.where(on, A[hh][i][j] + wgt[1 - hh] * pp, A[hh][i][j])
                    on = use if i == DIM - 1 else use1
                    for hh in (0, 1):
                        u = wgt[1 - hh] * phi[i]
                        for ch in range(3):
                            b[hh][i][ch] = np.where(on, b[hh][i][ch] + u * cq[hh][..., ch], b[hh][i][ch])
        # ---- the solve, per half
        o = []
        for hh in (0, 1):
            Ah, bh = A[hh], b[hh]
            sw = Ah[7][7]
            zero = [bh[7][ch] / sw for ch in range(3)]
            for j in range(7):
                Ah[j][j] = Ah[j][j] + ridge * sw
            good = np.ones((h, w), bool)
            for k in range(7):
                d = Ah[k][k]
                good = good & finite(d) & (d > F(0.0))
                for i in range(k + 1, DIM):
                    l = Ah[k][i] / d
                    for j in range(i, DIM):
                        Ah[i][j] = Ah[i][j] - l * Ah[k][j]
                    for ch in range(3):
                        bh[i][ch] = bh[i][ch] - l * bh[k][ch]
            d7 = Ah[7][7]
            good = good & finite(d7) & (d7 > F(0.0))
            beta = [bh[7][ch] / d7 for ch in range(3)]
            bfin = finite(beta[0]) & finite(beta[1]) & finite(beta[2])
            solved = hit & good & bfin
            count["fallback_pivot"] += int((valid & hit & ~good).sum())
            count["fallback_beta"] += int((valid & hit & good & ~bfin).sum())
            count["solved"] += int((valid & solved).sum())
            oh = np.stack([np.where(solved, beta[ch], zero[ch]) for ch in range(3)], -1)
            assert oh.dtype == np.float32
            o.append(oh / F(1.0))
        o0, o1 = o
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

FEATS = {"nan_normal": (3, 9), "inf_depth": (5, 17), "zero_depth": (6, 25), "huge_normal": (1, 28)}
HUGE = (slice(2, 7), slice(20, 29))               # both halves (3e38, 3e38, 3e38, 3): identical means of 1e38, V = 0 inside


def oracle_planes(count, w, h):
    return oracle_samples(count, w, h)[1]


def planted_features():
    """The oracle's 33 x 9 planes with four records planted: a NaN in a normal, an inf in a position's w, a position
    w = 0 at a hit (its own phi_6 is 0 / 0: the pixel accepts no tap), and a normal of 1e20, whose square overflows A."""
    p = {k: v.copy() for k, v in oracle_planes(6, 33, 9).items() if k in ("position", "normal", "albedo")}
    p["normal"][FEATS["nan_normal"]][1] = np.nan
    p["position"][FEATS["inf_depth"]][3] = np.inf
    p["position"][FEATS["zero_depth"]][3] = 0.0
    p["normal"][FEATS["huge_normal"]][0] = 1e20
    return p


def case(name):
    """(half0, half1, planes) of a named frame."""
    if name == "a":                 # 100 x 37, 16 samples
        return (*frame("a"), oracle_planes(16, W, H))
    if name in ("b6", "b5", "planted", "identical"):       # 33 x 9
        return (*frame(name), oracle_planes(6, 33, 9))
    if name == "strip":             # 70 x 3
        return (*frame("strip"), oracle_planes(4, 70, 3))
    if name == "one":               # 1 x 1
        return (*frame("one"), oracle_planes(4, 1, 1))
    if name == "planted_syn":       # the planted halves on planes with miss regions and near-zero albedo
        return (*frame("planted"), synthetic_frame(33, 9, 13)[1])
    if name == "b6_feat":           # the planted feature records
        return (*frame("b6"), planted_features())
    if name == "huge":              # colour sums that overflow b while A stays finite: beta is not finite
        h0, h1 = (a.copy() for a in frame("b6"))
        h0[HUGE] = (3e38, 3e38, 3e38, 3.0)
        h1[HUGE] = (3e38, 3e38, 3e38, 3.0)
        return h0, h1, oracle_planes(6, 33, 9)
    raise KeyError(name)


FRAMES = ("a", "b6", "b5", "strip", "one", "planted", "planted_syn", "b6_feat", "huge")
CASES = [(name, rf) for name in FRAMES for rf in RADII]
_want = {}


def expected(name, rf):
    """np_regress of a frame at (r, f), computed once (the GPU tests ask for the same ones)."""
    if (name, rf) not in _want:
        _want[name, rf] = np_regress(*case(name), search_radius=rf[0], patch_radius=rf[1])
    return _want[name, rf]


def assert_regress_equal(got, want, what):
    assert_images_equal(got[0], want[0], f"{what}: image")
    assert_images_equal(got[1], want[1], f"{what}: err")


def constant_planes(w, h):
    """Every pixel a hit with the same feature record."""
    full = lambda rec: np.broadcast_to(np.array(rec, np.float32), (h, w, 4)).copy()
    return {"position": full((0.5, -1.0, 2.0, 3.25)), "normal": full((0.6, 0.0, -0.8, 0.0)), "albedo": full((0.7, 0.01, 0.3, 1.0))}


# ---- 1. symbols and defaults -----------------------------------------------------------------------

NEW_SYMBOLS = ("surf_regress_default_params", "surf_denoise_regress", "surf_denoise_regress_copy_device", "surf_denoise_regress_image",
               "surf_denoise_regress_image_host", "surf_debug_regress_time")


def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("RegressParams", "regress_params", "denoise_regress_image_host"):
        assert hasattr(surf_amd, name), name
    for name in ("denoise_regress", "denoise_regress_image", "copy_denoise_regress_to", "debug_regress_time"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_params():
    p = surf_amd.RegressParams()
    assert C.sizeof(p) == 24
    p.search_radius, p.k, p.ridge = 9, 7.0, 3.0
    assert surf_amd.load().surf_regress_default_params(C.byref(p)) == 0
    assert (p.search_radius, p.patch_radius) == (5, 2)
    assert (F(p.k), F(p.alpha), F(p.eps), F(p.ridge)) == (F(0.7), F(1.0), F(1e-10), F(0.1))
    assert {k: F(getattr(p, k)) for k in DEFAULTS} == {k: F(v) for k, v in DEFAULTS.items()}
    q = surf_amd.regress_params(search_radius=3, ridge=0.01)
    assert (q.search_radius, q.patch_radius, F(q.k), F(q.ridge)) == (3, 2, F(0.7), F(0.01))
    with pytest.raises(TypeError):
        surf_amd.regress_params(sigma=1.0)


# ---- 2. status codes ---------------------------------------------------------------------------------

def test_invalid_arguments_are_status_codes():
    lib = surf_amd.load()
    h0, h1, planes = case("b5")
    h, w = h0.shape[:2]
    out, err = np.zeros_like(h0), np.zeros_like(h0)
    good = surf_amd.regress_params(search_radius=1, patch_radius=0)
    gb = C.byref(good)
    host = lib.surf_denoise_regress_image_host
    a, b, o, e = h0.ctypes.data, h1.ctypes.data, out.ctypes.data, err.ctypes.data
    P, N, A = (np.ascontiguousarray(planes[k]).ctypes.data for k in ("position", "normal", "albedo"))
    assert host(w, h, a, b, P, N, A, gb, o, e) == 0
    assert host(w, h, a, b, P, N, A, gb, o, None) == 0                          # the error image is optional
    for bad in ((w, h, None, b, P, N, A, gb, o, e), (w, h, a, None, P, N, A, gb, o, e), (w, h, a, b, None, N, A, gb, o, e),
                (w, h, a, b, P, None, A, gb, o, e), (w, h, a, b, P, N, None, gb, o, e), (w, h, a, b, P, N, A, None, o, e),
                (w, h, a, b, P, N, A, gb, None, e), (0, h, a, b, P, N, A, gb, o, e), (w, 0, a, b, P, N, A, gb, o, e)):
        assert host(*bad) == SURF_ERR_INVALID, bad
    nan, inf = float("nan"), float("inf")
    for field, values in (("search_radius", (0, 11)), ("patch_radius", (4,)), ("k", (0.0, nan, inf, -1.0)), ("alpha", (-1.0, -1e-30, nan, inf)),
                          ("eps", (0.0, -1.0, nan, inf)), ("ridge", (0.0, -1.0, nan, inf))):
        for val in values:
            p = surf_amd.regress_params(**{"search_radius": 1, "patch_radius": 0, field: val})
            assert host(w, h, a, b, P, N, A, C.byref(p), o, e) == SURF_ERR_INVALID, (field, val)
    for field, values in (("search_radius", (1, 10)), ("patch_radius", (0, 3)), ("k", (1e-3, 10.0)), ("alpha", (0.0, 4.0)), ("eps", (1e-30, 1.0)),
                          ("ridge", (1e-30, 100.0))):
        for val in values:
            p = surf_amd.regress_params(**{"search_radius": 1, "patch_radius": 0, field: val})
            assert host(w, h, a, b, P, N, A, C.byref(p), o, e) == 0, (field, val)
    with pytest.raises(surf_amd.SurfError) as ex:
        surf_amd.denoise_regress_image_host(h0, h1, planes, ridge=0.0)
    assert ex.value.code == SURF_ERR_INVALID and "ridge" in str(ex.value)
    with pytest.raises(ValueError):
        surf_amd.denoise_regress_image_host(h0, h1[:, :5], planes)
    with pytest.raises(ValueError):
        surf_amd.denoise_regress_image_host(h0, h1, [planes["position"], planes["normal"][:, :5], planes["albedo"]])
    # a NULL context
    ms = (C.c_float * 3)()
    assert lib.surf_regress_default_params(None) == SURF_ERR_INVALID
    assert lib.surf_denoise_regress(None, gb, o, e) == SURF_ERR_INVALID
    assert lib.surf_denoise_regress_copy_device(None, gb, o, e) == SURF_ERR_INVALID
    assert lib.surf_denoise_regress_image(None, w, h, a, b, P, N, A, gb, o, e) == SURF_ERR_INVALID
    assert lib.surf_debug_regress_time(None, ms, 3) == SURF_ERR_INVALID


# ---- 3. the host twin equals numpy, bit for bit ----------------------------------------------------

@pytest.mark.parametrize("name,rf", CASES, ids=[f"{n}-r{r}f{f}" for n, (r, f) in CASES])
def test_host_twin_bitexact(name, rf):
    h0, h1, planes = case(name)
    want = expected(name, rf)
    print(f"{name} {h0.shape[1]} x {h0.shape[0]}, r {rf[0]}, f {rf[1]}: {want[2]}")
    got = surf_amd.denoise_regress_image_host(h0, h1, planes, search_radius=rf[0], patch_radius=rf[1])
    assert_regress_equal(got, want, f"{name}, r {rf[0]}, f {rf[1]}")


OTHER_SCALARS = (dict(k=1.0, alpha=0.0, ridge=0.01), dict(k=0.2, alpha=2.0, eps=1e-4, ridge=1.0))


def test_other_scalars_bitexact():
    """k, alpha, eps and ridge away from their defaults, alpha = 0 (no variance cancellation) among them."""
    h0, h1, planes = case("b5")
    for kw in OTHER_SCALARS:
        sp = dict(search_radius=3, patch_radius=1, **kw)
        assert_regress_equal(surf_amd.denoise_regress_image_host(h0, h1, planes, **sp), np_regress(h0, h1, planes, **sp), str(kw))


# ---- 4. the inputs reach every branch ----------------------------------------------------------------

def test_inputs_reach_every_branch():
    total = {}
    for name, rf in CASES:
        for k, v in expected(name, rf)[2].items():
            total[k] = total.get(k, 0) + v
    print(total)
    for k in BRANCHES:
        assert total[k] > 0, k
    # what each planted record is there for
    cnt = expected("b6_feat", (5, 2))[2]
    assert cnt["nonfinite_tap"] > 0 and cnt["fallback_pivot"] > 0 and cnt["miss_tap"] == 0
    out = expected("b6_feat", (5, 2))[0]
    for k in ("zero_depth", "nan_normal", "inf_depth"):                            # a centre whose own record is not finite: no tap, 0 / 0
        assert np.isnan(out[FEATS[k]][:3]).all(), k
    assert np.isfinite(out[FEATS["huge_normal"]]).all()                            # the pivot overflows: order zero
    cnt = expected("planted_syn", (5, 2))[2]
    assert cnt["miss_tap"] > 0 and cnt["miss_centre"] > 0 and cnt["invalid_pixel"] == 3 and cnt["invalid_tap"] > 0
    assert expected("huge", (1, 0))[2]["fallback_beta"] > 0


# ---- 5. constant planes: the non-local-means filter, bit for bit -----------------------------------

@pytest.mark.parametrize("name", ["a", "b5"])
@pytest.mark.parametrize("rf", [(3, 1), (5, 2)], ids=["r3f1", "r5f2"])
def test_constant_planes_give_non_local_means(name, rf):
    h0, h1 = frame(name)
    planes = constant_planes(h0.shape[1], h0.shape[0])
    sp = dict(search_radius=rf[0], patch_radius=rf[1], k=DEFAULTS["k"])
    want = np_nlm(h0, h1, **sp)
    assert_regress_equal(np_regress(h0, h1, planes, **sp), want, f"np_regress on constant planes, {name}, {rf}")
    assert_regress_equal(surf_amd.denoise_regress_image_host(h0, h1, planes, **sp), want, f"the twin on constant planes, {name}, {rf}")
    assert_regress_equal(surf_amd.denoise_nlm_image_host(h0, h1, **sp), want, f"the non-local-means twin, {name}, {rf}")


def test_identical_halves_have_no_error():
    h0, h1, planes = case("identical")
    want = np_regress(h0, h1, planes)
    assert not want[1].any()
    assert_regress_equal(surf_amd.denoise_regress_image_host(h0, h1, planes), want, "identical halves")


# ---- 6. quality ------------------------------------------------------------------------------------

RATIO_64 = 1.10      # np_regress measures 0.9545 against np_nlm; x 1.15, rounded up to two decimals


def test_regression_against_non_local_means():
    """The oracle's indoor scene at 100 x 37, spp-1 frames from frame 0 through two buckets, mean absolute error
    over all pixels against the oracle's 2048-spp render of the same view (first_frame 100000), set up as
    test_sampled_host.quality sets it up: np_regress against np_nlm on the same halves, each at its own
    defaults -- both restatements, never the library.  Conditions: the regression's error is below the noisy
    mean's at 16 and at 64 samples, and below non-local means' at 16.  At 64 the asserted ratio is np_regress's
    measured one x 1.15, rounded up to two decimals (test_sampled_host's RATIO_64 convention; the margin is for
    parameter retuning, the result is deterministic).  N = 4 is printed, not asserted.  np_regress measures
    (MEASUREMENTS "First-order regression"), noisy / non-local means / regression, ratio:
    N = 4   0.06107 / 0.01864 / 0.01573, 0.8437;
    N = 16  0.03749 / 0.01388 / 0.01263, 0.9099, asserted < 1;
    N = 64  0.02164 / 0.01039 / 0.00992, 0.9545, asserted <= 1.10."""
    res = quality((16, 64), 2048)
    ref = reference()
    mae = lambda img: float(np.abs(img[..., :3].astype(np.float64) - ref).mean())
    planes = oracle_planes(64, W, H)
    got = {}
    for n in (4, 16, 64):
        h0, h1 = halves(n)
        noisy = res[n][0] if n in res else mae((h0 + h1) / (h0 + h1)[..., 3:4])
        nlm, fit = np_nlm(h0, h1)[0], np_regress(h0, h1, planes)[0]
        got[n] = (noisy, mae(nlm), mae(fit), fit, h0, h1)
        print(f"N = {n}: noisy {noisy:.5f}, non-local means {got[n][1]:.5f}, regression {got[n][2]:.5f}, ratio {got[n][2] / got[n][1]:.4f}")
    noisy, nlm, fit, want, h0, h1 = got[64]
    assert_images_equal(surf_amd.denoise_regress_image_host(h0, h1, planes)[0], want, "the host twin at 64 samples")
    assert got[16][2] < got[16][0] and fit < noisy, (got[16], fit, noisy)
    assert got[16][2] / got[16][1] < 1.0, (got[16][2], got[16][1])
    assert fit / nlm <= RATIO_64, (fit / nlm, fit, nlm)
