"""The display stage (surf_display*, include/surf_hip.h) where it needs no GPU: exported
symbols and defaults, status codes, the two tables, the CPU twin against a numpy
restatement, the branches the inputs reach, independent checks of the meter and the
stage's properties.  CPU only.

Bar: bit-exact, RGBA8 words and every field of the meter's result.  The expected images
never come from the code under test: np_display below restates the header's rules 1-8,
every step an explicit float32 numpy operation in the stated order; expf is glibc's, the
Bayer matrix is written out, the sRGB table is computed in float64 numpy (an entry where
the C library's pow rounds differently from numpy's may be taken from the export after it
is shown to lie within one f32 ulp; SRGB_FROM_EXPORT names those entries).

tests/test_gpu_display.py imports the restatement, the frames and the parameters from here.
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from test_denoise_host import glibc_expf
from test_sampled_host import H, W, np_squares, oracle_samples

F = np.float32
SURF_ERR_INVALID = -1
DEFAULTS = dict(exposure_mode=1, exposure=1.0, key=0.18, min_scale=1.0 / 64.0, max_scale=64.0, bloom_radius=0, bloom_threshold=1.0,
                bloom_strength=0.1, curve=2, white=4.0, transfer=2, dither=1)
BAYER8 = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
                   [48, 16, 56, 24, 50, 18, 58, 26],
                   [12, 44, 4, 36, 14, 46, 6, 38],
                   [60, 28, 52, 20, 62, 30, 54, 22],
                   [3, 35, 11, 43, 1, 33, 9, 41],
                   [51, 19, 59, 27, 49, 17, 57, 25],
                   [15, 47, 7, 39, 13, 45, 5, 37],
                   [63, 31, 55, 23, 61, 29, 53, 21]], np.uint8)
FIRST_BIN = 888                                   # bits(2^-16) >> 20


def np_srgb_table():
    """Rule 7's table in float64 numpy, rounded to f32."""
    r = np.arange(4096, dtype=np.float64) / 4095.0
    l = r * r
    with np.errstate(all="ignore"):
        return np.where(l <= 0.0031308, 12.92 * l, 1.055 * np.power(l, 1.0 / 2.4) - 0.055).astype(np.float32)


def srgb_against_export():
    """(the numpy table, the export, the entries where they differ)."""
    mine, lib = np_srgb_table(), surf_amd.display_srgb_table()
    return mine, lib, np.flatnonzero(mine.view(np.uint32) != lib.view(np.uint32))


_table = {}


def srgb_table():
    """The table np_display reads: numpy's, with the entries where libm's pow rounds the other way (each within one f32
    ulp, test_srgb_table) taken from the export."""
    if "T" not in _table:
        mine, lib, differ = srgb_against_export()
        T = mine.copy()
        T[differ] = lib[differ]
        T.setflags(write=False)
        _table["T"] = T
    return _table["T"]


def np_display(img, **params):
    """The header's arithmetic on an (H, W, 4) float RGBA image.  Returns (words (H, W) uint32, the meter's result as
    a dict, counts of the branches taken)."""
    sp = {**DEFAULTS, **params}
    assert set(params) <= set(DEFAULTS)
    A = np.ascontiguousarray(img, np.float32)
    h, w = A.shape[:2]
    cnt = {}
    with np.errstate(all="ignore"):
        # 1. colour
        n = A[..., 3]
        has = n > F(0.0)
        c = np.where(has[..., None], A[..., :3] / n[..., None], F(0.0)).astype(np.float32)
        keep = c > F(0.0)
        cnt["no_weight"] = int((~has).sum())
        cnt["nan"] = int(np.isnan(c).sum())
        cnt["negative"] = int((c < F(0.0)).sum())
        cnt["inf"] = int(np.isposinf(c).sum())
        cnt["kept"] = int(keep.sum())
        c = np.where(keep, c, F(0.0)).astype(np.float32)
        # 2. luminance
        L = np.ascontiguousarray((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2])
        assert L.dtype == np.float32
        # 3. meter
        b = (L.view(np.uint32) >> 20).astype(np.int64)
        black = b < FIRST_BIN
        bins = b[~black] - FIRST_BIN
        cnt["bin_capped"] = int((bins > 255).sum())
        cnt["bin_plain"] = int((bins <= 255).sum())
        cnt["black"] = int(black.sum())
        hist = np.bincount(np.minimum(bins, 255), minlength=256).astype(np.uint32)
        counted = int(hist.sum())
        cum = np.cumsum(hist.astype(np.uint64))
        m = int(np.argmax(2 * cum >= np.uint64(counted)))                  # the first bin that reaches half
        Lm = np.array([((m + FIRST_BIN) << 20) | 0x80000], np.uint32).view(np.float32)[0]
        if sp["exposure_mode"] == 0:
            scale = F(sp["exposure"])
            cnt["manual"] = 1
        elif counted == 0:
            scale = F(1.0)
            cnt["counted_0"] = 1
        else:
            scale = F(sp["key"]) / Lm
            lo, hi = scale < F(sp["min_scale"]), scale > F(sp["max_scale"])
            scale = F(sp["min_scale"]) if lo else scale
            scale = F(sp["max_scale"]) if scale > F(sp["max_scale"]) else scale
            cnt["scale_min" if lo else "scale_max" if hi else "scale_between"] = 1
        assert scale.dtype == np.float32
        meter = {"hist": hist, "counted": counted, "black": int(black.sum()), "median_bin": m, "scale": scale}
        # 4. exposed colour
        e = c * scale
        # 5. bloom
        R = int(sp["bloom_radius"])
        x = e
        if R > 0:
            sigma = F(0.5) * F(R)
            g = glibc_expf(np.array([-F(i * i) / (F(2.0) * sigma * sigma) for i in range(R + 1)], np.float32))
            S = g[0]
            for i in range(1, R + 1):
                S = S + (g[i] + g[i])
            wn = g / S
            assert wn.dtype == np.float32
            d = e - F(sp["bloom_threshold"])
            bright = d > F(0.0)
            cnt["bright"] = int(bright.sum())
            cnt["not_bright"] = int((~bright).sum())
            B = np.where(bright, d, F(0.0)).astype(np.float32)
            xs, ys = np.arange(w), np.arange(h)
            Hh = np.zeros((h, w, 3), np.float32)
            for i in range(-R, R + 1):
                Hh = Hh + wn[abs(i)] * B[:, np.clip(xs + i, 0, w - 1)]
            Vv = np.zeros((h, w, 3), np.float32)
            for j in range(-R, R + 1):
                Vv = Vv + wn[abs(j)] * Hh[np.clip(ys + j, 0, h - 1)]
            x = e + F(sp["bloom_strength"]) * Vv
            assert x.dtype == np.float32
        # 6. curve
        if sp["curve"] == 0:
            t = x
        elif sp["curve"] == 1:
            t = (x * (F(1.0) + x / (F(sp["white"]) * F(sp["white"])))) / (F(1.0) + x)
        else:
            t = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        below = t < F(1.0)
        cnt["curve_nan"] = int(np.isnan(t).sum())
        cnt["curve_above_1"] = int((t >= F(1.0)).sum())
        v = np.where(below, t, F(1.0)).astype(np.float32)
        positive = v > F(0.0)
        cnt["curve_zero"] = int((~positive).sum())
        cnt["curve_between"] = int((below & positive).sum())
        v = np.where(positive, v, F(0.0)).astype(np.float32)
        # 7. transfer
        if sp["transfer"] == 0:
            u = v
        elif sp["transfer"] == 1:
            u = np.sqrt(v)
        else:
            u = srgb_table()[(np.sqrt(v) * F(4095.0) + F(0.5)).astype(np.uint32)]
        assert u.dtype == np.float32
        # 8. quantise
        yy, xx = np.meshgrid(np.arange(h) & 7, np.arange(w) & 7, indexing="ij")
        d = (BAYER8[yy, xx].astype(np.float32) + F(0.5)) / F(64.0) if sp["dither"] else np.full((h, w), F(0.5), np.float32)
        assert d.dtype == np.float32
        qf = u * F(255.0) + d[..., None]
        q = qf.astype(np.uint32)
        cnt["q_capped"] = int((q > 255).sum())
        q = np.minimum(q, 255).astype(np.uint32)
    words = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(255 << 24)
    return words.astype(np.uint32), meter, cnt


# ---- the inputs ----------------------------------------------------------------------------------

_cache = {}


def accumulator(count, w=W, h=H):
    """The f32 sum of the oracle's first `count` samples at w x h (w = count everywhere); computed once, read only."""
    key = (count, w, h)
    if key not in _cache:
        a = np_squares(oracle_samples(count, w, h)[0])[0]
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def grey_with_luminance(target_bits):
    """A grey level g whose luminance (rule 2) has exactly the bits `target_bits`."""
    for k in range(-16, 17):
        g = np.array([target_bits + k], np.uint32).view(np.float32)[0]
        L = (F(0.2126) * g + F(0.7152) * g) + F(0.0722) * g
        if L.view(np.uint32) == target_bits:
            return g
    raise AssertionError(f"no grey level has the luminance bits {target_bits:#x}")


EDGE = FIRST_BIN << 20                              # the bits of 2^-16
PLANTED = {"empty": (1, 3), "nan": (4, 8), "inf": (7, 12), "negative": (2, 16), "huge": (5, 20), "edge": (3, 24), "below": (3, 25),
           "bright": (6, 28)}


def planted():
    """The 33 x 9 frame of 6 samples with: a pixel of weight 0; a NaN, a +inf, a negative and a 3e38 channel; a pixel of
    exactly 2^-16 luminance and one a bit below it; one pixel of luminance >= 2^16."""
    a = accumulator(6, 33, 9).copy()
    a[PLANTED["empty"]][3] = 0.0
    a[PLANTED["nan"]][1] = np.nan
    a[PLANTED["inf"]][0] = np.inf
    a[PLANTED["negative"]][2] = -4.0
    a[PLANTED["huge"]][1] = 3e38
    for name, bits in (("edge", EDGE), ("below", EDGE - 1)):
        g = grey_with_luminance(bits)
        a[PLANTED[name]] = (g, g, g, 1.0)
    a[PLANTED["bright"]] = (70000.0, 70000.0, 70000.0, 1.0)
    return a


def frame(name):
    if name == "a":                 # 100 x 37, 16 samples
        return accumulator(16)
    if name == "b":                 # 33 x 9, 6 samples: no multiple of the tile, lower than the blur window at R = 16
        return accumulator(6, 33, 9)
    if name == "strip":             # 70 x 3: narrower in y than every blur window but R = 1's
        return accumulator(4, 70, 3)
    if name == "one":               # 1 x 1: every tap clamps to the one pixel
        return accumulator(4, 1, 1)
    if name == "planted":
        return planted()
    if name == "black":             # nothing above 2^-16: counted = 0, scale = 1
        a = np.zeros((5, 7, 4), np.float32)
        a[..., 3] = 2.0
        a[2, 3, :3] = 1e-6
        return a
    raise KeyError(name)


FRAMES = ("a", "b", "strip", "one", "planted", "black")
PSETS = {
    "defaults": {},
    "key_low": dict(key=1e-4),                                  # the quotient ends below min_scale
    "key_high": dict(key=100.0),                                # ... above max_scale
    "manual_quarter": dict(exposure_mode=0, exposure=0.25, curve=0, transfer=0, dither=0),
    "manual_7": dict(exposure_mode=0, exposure=7.0, curve=1, transfer=1, dither=1),
    "none_srgb": dict(curve=0, transfer=2, dither=0),
    "reinhard_linear": dict(curve=1, white=2.0, transfer=0, dither=1),
    "aces_sqrt": dict(curve=2, transfer=1, dither=0),
    "bloom_0_t0": dict(bloom_radius=0, bloom_threshold=0.0),
    "bloom_1_t0": dict(bloom_radius=1, bloom_threshold=0.0, bloom_strength=0.5),
    "bloom_1_t1": dict(bloom_radius=1, bloom_threshold=1.0, bloom_strength=1.0),
    "bloom_4_t0": dict(bloom_radius=4, bloom_threshold=0.0),
    "bloom_4_t1": dict(bloom_radius=4, bloom_threshold=1.0, bloom_strength=0.5, curve=1, dither=0),
    "bloom_16_t0": dict(bloom_radius=16, bloom_threshold=0.0, exposure_mode=0, exposure=2.0),
    "bloom_16_t1": dict(bloom_radius=16, bloom_threshold=1.0, bloom_strength=2.0),
}
CASES = [(f, s) for f in FRAMES for s in PSETS]
_want = {}


def expected(name, pset):
    """np_display of a frame under a parameter set, computed once (the GPU tests ask for the same ones)."""
    if (name, pset) not in _want:
        _want[name, pset] = np_display(frame(name), **PSETS[pset])
    return _want[name, pset]


METER_FIELDS = ("counted", "black", "median_bin")


def assert_display_equal(got, want, what):
    """(words, meter) against np_display's, bit for bit."""
    words, meter = got
    assert words.shape == want[0].shape and words.dtype == np.uint32, f"{what}: {words.shape} {words.dtype}"
    bad = np.argwhere(words != want[0])
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first (row, x) {bad[:4].tolist()}: "
                           f"got {words[tuple(bad[0])]:#010x}, want {want[0][tuple(bad[0])]:#010x}")
    if meter is None:
        return
    assert np.array_equal(meter["hist"], want[1]["hist"]), f"{what}: hist"
    for k in METER_FIELDS:
        assert meter[k] == want[1][k], (what, k, meter[k], want[1][k])
    assert F(meter["scale"]).view(np.uint32) == F(want[1]["scale"]).view(np.uint32), (what, meter["scale"], want[1]["scale"])


# ---- 1. symbols and defaults -----------------------------------------------------------------------

NEW_SYMBOLS = ("surf_display_default_params", "surf_display", "surf_display_image", "surf_display_image_device", "surf_display_image_host",
               "surf_display_srgb_table", "surf_display_bayer8", "surf_debug_display_time")


def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("DisplayParams", "DisplayMeterResult", "display_params", "display_default_params", "display_image_host",
                 "display_srgb_table", "display_bayer8"):
        assert hasattr(surf_amd, name), name
    for name in ("display", "display_image", "display_image_device", "debug_display_time"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_params():
    p = surf_amd.DisplayParams()
    assert C.sizeof(p) == 48 and C.sizeof(surf_amd.DisplayMeterResult) == 1040
    p.curve, p.key, p.bloom_radius = 9, 7.0, 3
    assert surf_amd.load().surf_display_default_params(C.byref(p)) == 0
    for k, v in DEFAULTS.items():
        got = getattr(p, k)
        assert (got == v) if isinstance(v, int) else (F(got) == F(v)), (k, got, v)
    d = surf_amd.display_default_params()
    assert bytes(d) == bytes(p)
    q = surf_amd.display_params(bloom_radius=4, white=2.0)
    assert (q.bloom_radius, F(q.white), q.curve, F(q.key)) == (4, F(2.0), 2, F(0.18))
    with pytest.raises(TypeError):
        surf_amd.display_params(gamma=2.2)


# ---- 2. status codes ---------------------------------------------------------------------------------

def test_invalid_arguments_are_status_codes():
    lib = surf_amd.load()
    img = frame("b")
    h, w = img.shape[:2]
    out = np.zeros((h, w), np.uint32)
    meter = surf_amd.DisplayMeterResult()
    good = surf_amd.display_params()
    gb, mb = C.byref(good), C.byref(meter)
    host = lib.surf_display_image_host
    a, o = img.ctypes.data, out.ctypes.data
    assert host(w, h, a, gb, o, mb) == 0
    assert host(w, h, a, gb, o, None) == 0                                      # the meter's result is optional
    for bad in ((w, h, None, gb, o, mb), (w, h, a, None, o, mb), (w, h, a, gb, None, mb), (0, h, a, gb, o, mb), (w, 0, a, gb, o, mb),
                (1 << 14, (1 << 13) + 1, a, gb, o, mb)):
        assert host(*bad) == SURF_ERR_INVALID, bad
    nan, inf = float("nan"), float("inf")
    positive, nonneg = (0.0, -1.0, nan, inf), (-1.0, -1e-30, nan, inf)
    for field, values in (("exposure_mode", (2,)), ("exposure", positive), ("key", positive), ("min_scale", positive + (65.0,)),
                          ("max_scale", positive + (1.0 / 128.0,)), ("bloom_radius", (17,)), ("bloom_threshold", nonneg),
                          ("bloom_strength", nonneg), ("curve", (3,)), ("white", positive), ("transfer", (3,)), ("dither", (2,))):
        for val in values:
            p = surf_amd.display_params(**{field: val})
            assert host(w, h, a, C.byref(p), o, mb) == SURF_ERR_INVALID, (field, val)
    for field, values in (("exposure_mode", (0, 1)), ("exposure", (1e-30, 1e30)), ("key", (1e-30, 1e30)), ("min_scale", (1e-30, 64.0)),
                          ("max_scale", (1.0 / 64.0, 1e30)), ("bloom_radius", (0, 16)), ("bloom_threshold", (0.0, 1e30)),
                          ("bloom_strength", (0.0, 1e30)), ("curve", (0, 1, 2)), ("white", (1e-30, 1e30)), ("transfer", (0, 1, 2)),
                          ("dither", (0, 1))):
        for val in values:
            p = surf_amd.display_params(**{field: val})
            assert host(w, h, a, C.byref(p), o, mb) == 0, (field, val)
    with pytest.raises(surf_amd.SurfError) as ex:
        surf_amd.display_image_host(img, bloom_radius=17)
    assert ex.value.code == SURF_ERR_INVALID and "bloom_radius" in str(ex.value)
    with pytest.raises(ValueError):
        surf_amd.display_image_host(img[..., :3])
    # a NULL context, NULL tables
    ms = (C.c_float * 4)()
    assert lib.surf_display_default_params(None) == SURF_ERR_INVALID
    assert lib.surf_display(None, gb, o, mb) == SURF_ERR_INVALID
    assert lib.surf_display_image(None, w, h, a, gb, o, mb) == SURF_ERR_INVALID
    assert lib.surf_display_image_device(None, w, h, a, gb, o, mb) == SURF_ERR_INVALID
    assert lib.surf_debug_display_time(None, ms, 4) == SURF_ERR_INVALID
    assert lib.surf_display_srgb_table(None) == SURF_ERR_INVALID
    assert lib.surf_display_bayer8(None) == SURF_ERR_INVALID


# ---- 3. the tables ---------------------------------------------------------------------------------

SRGB_FROM_EXPORT = ()        # the entries where libm's pow and numpy's round differently: none on glibc 2.35 with numpy's float64 power


def test_bayer_matrix():
    assert np.array_equal(surf_amd.display_bayer8(), BAYER8)
    assert sorted(BAYER8.ravel().tolist()) == list(range(64))


def test_srgb_table():
    mine, lib, differ = srgb_against_export()
    print("entries that differ:", differ.tolist())
    assert tuple(differ.tolist()) == SRGB_FROM_EXPORT
    if len(differ):
        assert (np.abs(mine.view(np.int32)[differ] - lib.view(np.int32)[differ]) <= 1).all()
    assert lib[0] == 0.0 and lib[4095] == 1.0 and (np.diff(lib) > 0).all()
    # indexed by the square root, the steepest step of the table is well below a tenth of an 8-bit code in the dark part
    dark = lib[: int(np.sqrt(0.05) * 4095)]
    assert np.diff(dark).max() * 255.0 < 0.2 and np.diff(lib).max() * 255.0 < 0.2


# ---- 4. the host twin equals numpy, bit for bit ----------------------------------------------------

@pytest.mark.parametrize("name,pset", CASES, ids=[f"{f}-{s}" for f, s in CASES])
def test_host_twin_bitexact(name, pset):
    want = expected(name, pset)
    print(f"{name} {pset}: scale {want[1]['scale']}, median bin {want[1]['median_bin']}, {want[2]}")
    assert_display_equal(surf_amd.display_image_host(frame(name), **PSETS[pset]), want, f"{name}, {pset}")


def test_frames_are_what_they_claim():
    assert frame("a").shape == (37, 100, 4) and (frame("a")[..., 3] == 16).all()
    assert frame("b").shape == (9, 33, 4) and frame("strip").shape == (3, 70, 4) and frame("one").shape == (1, 1, 4)
    a = frame("planted")
    assert a[PLANTED["empty"]][3] == 0 and np.isnan(a[PLANTED["nan"]]).sum() == 1 and np.isinf(a[PLANTED["inf"]]).sum() == 1
    assert a[PLANTED["negative"]][2] < 0 and a[PLANTED["huge"]][1] == F(3e38)
    lum = lambda px: (F(0.2126) * px[0] + F(0.7152) * px[1]) + F(0.0722) * px[2]
    assert lum(a[PLANTED["edge"]]) == F(2.0 ** -16) and lum(a[PLANTED["below"]]) < F(2.0 ** -16) and lum(a[PLANTED["bright"]]) >= F(2.0 ** 16)


# ---- 5. the inputs reach every branch ----------------------------------------------------------------

def test_inputs_reach_every_branch():
    total = {}
    for name, pset in CASES:
        for k, v in expected(name, pset)[2].items():
            total[k] = total.get(k, 0) + v
    print(total)
    for k in ("no_weight", "nan", "negative", "inf", "kept", "bin_capped", "bin_plain", "black", "manual", "counted_0", "scale_min",
              "scale_max", "scale_between", "bright", "not_bright", "curve_nan", "curve_above_1", "curve_zero", "curve_between"):
        assert total[k] > 0, k
    # rule 8's cap at 255 cannot bind: u <= 1 and d < 1, so u * 255 + d < 256 for every input; the rule stays as stated
    assert total["q_capped"] == 0
    # what each planted record is there for, at the defaults
    words, meter, cnt = expected("planted", "defaults")
    assert cnt["no_weight"] == 1 and cnt["nan"] == 1 and cnt["negative"] == 1 and cnt["inf"] == 1
    plain = expected("b", "defaults")[1]
    assert meter["black"] == plain["black"] + 2                                       # the empty pixel and the one just below 2^-16
    assert meter["hist"][0] == plain["hist"][0] + 1                                   # exactly 2^-16: the first bin
    assert meter["hist"][255] == plain["hist"][255] + 3                               # +inf, 3e38 and 70000 land in the last bin
    assert words[PLANTED["empty"]] == 0xFF000000 and words[PLANTED["inf"]] & 0xFF == 0xFF and words[PLANTED["huge"]] >> 8 & 0xFF == 0xFF
    assert expected("black", "defaults")[1]["counted"] == 0 and expected("black", "defaults")[1]["scale"] == F(1.0)
    assert expected("a", "key_low")[1]["scale"] == F(1.0 / 64.0) and expected("a", "key_high")[1]["scale"] == F(64.0)


# ---- 6. the meter, independently ---------------------------------------------------------------------

def test_meter_against_a_sort():
    a = frame("a")
    _, meter = surf_amd.display_image_host(a)
    c = np.maximum(a[..., :3] / a[..., 3:], F(0.0))
    L = ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).ravel()
    counted = np.sort(L[L >= F(2.0 ** -16)])
    assert meter["counted"] == len(counted) and meter["black"] == len(L) - len(counted)
    assert int(meter["hist"].astype(np.uint64).sum()) + meter["black"] == a.shape[0] * a.shape[1]
    mid = counted[(len(counted) + 1) // 2 - 1]
    assert meter["median_bin"] == min((int(mid.view(np.uint32)) >> 20) - FIRST_BIN, 255)
    lm = np.array([((meter["median_bin"] + FIRST_BIN) << 20) | 0x80000], np.uint32).view(np.float32)[0]
    assert meter["scale"] == F(0.18) / lm
    assert 2.0 ** -0.125 <= mid / lm <= 2.0 ** 0.125                                   # the bin's centre is within 1/8 octave of the median


# ---- 7. properties -----------------------------------------------------------------------------------

PLAIN = dict(exposure_mode=0, exposure=1.0, curve=0, transfer=0, dither=0)


def channels(words):
    return np.stack([(words >> s) & 0xFF for s in (0, 8, 16, 24)], -1)


def test_identity_is_the_rounded_clamp():
    a = frame("a")
    words, meter = surf_amd.display_image_host(a, **PLAIN)
    c = np.clip(a[..., :3] / a[..., 3:], F(0.0), F(1.0))
    want = np.floor(c * F(255.0) + F(0.5)).astype(np.uint32)
    got = channels(words)
    assert np.array_equal(got[..., :3], want) and (got[..., 3] == 255).all() and meter["scale"] == F(1.0)


def test_bloom_on_a_constant_image():
    """Below the threshold bloom changes nothing.  With threshold 0 and strength 1 a constant image c becomes c + Vv with
    Vv = c * (sum of wn)^2 up to rounding: each wn_i = g_i / S carries one rounding, S the R roundings of its sum, each
    pass 2 (2R + 1) more (a product and an addition per tap), so |Vv / c - 1| <= 2 * (3 (2R + 1) + R + 1) * 2^-24 to first
    order -- 4.1e-6 * 3.3 at R = 16, far from the half code that separates 0.4 * 255 + 0.5 = 102.5 from its neighbours."""
    const = np.zeros((20, 45, 4), np.float32)
    const[...] = (0.5, 0.5, 0.5, 1.0)
    for R in (1, 4, 16):
        off, _ = surf_amd.display_image_host(const, bloom_radius=0, **PLAIN)
        on, _ = surf_amd.display_image_host(const, bloom_radius=R, bloom_threshold=1.0, bloom_strength=3.0, **PLAIN)
        assert np.array_equal(on, off), R
    const[..., :3] = 0.2
    for R in (1, 4, 16):
        bound = 2 * (3 * (2 * R + 1) + R + 1) * 2.0 ** -24
        assert 0.2 * 255 * bound < 0.01
        words, _ = surf_amd.display_image_host(const, bloom_radius=R, bloom_threshold=0.0, bloom_strength=1.0, **PLAIN)
        assert (channels(words)[..., :3] == 102).all(), R


def test_scaling_the_records_changes_nothing():
    a = frame("a")
    for pset in ("defaults", "bloom_4_t1"):
        got = surf_amd.display_image_host(a * F(2.0 ** -20), **PSETS[pset])
        assert_display_equal(got, expected("a", pset), f"records scaled by 2^-20, {pset}")


def test_dither_splits_a_half_code_evenly():
    near = np.array([F(100.5) / F(255.0)], np.float32).view(np.uint32)[0] + np.arange(-8, 9, dtype=np.int64)
    near = near.astype(np.uint32).view(np.float32)
    c = near[near * F(255.0) == F(100.5)][0]                                           # u * 255 has the fraction 0.5 exactly
    img = np.zeros((16, 24, 4), np.float32)
    img[...] = (c, c, c, 1.0)
    words, _ = surf_amd.display_image_host(img, **{**PLAIN, "dither": 1})
    red = channels(words)[..., 0]
    for y0 in (0, 8):
        for x0 in (0, 8, 16):
            cell = red[y0:y0 + 8, x0:x0 + 8]
            assert (cell == 100).sum() == 32 and (cell == 101).sum() == 32, (y0, x0)
            assert np.array_equal(cell == 101, BAYER8 >= 32)
    flat, _ = surf_amd.display_image_host(img, **PLAIN)
    assert (channels(flat)[..., 0] == 101).all()                                       # without dither: floor(100.5 + 0.5)


def test_unaligned_plane():
    """The caller's plane need not be 16-byte aligned."""
    a = frame("b")
    raw = np.zeros(a.size + 1, np.float32)
    raw[1:] = a.ravel()
    assert_display_equal(surf_amd.display_image_host(raw[1:].reshape(a.shape)), expected("b", "defaults"), "a plane 4 bytes off")


# ---- 8. the conversion tool --------------------------------------------------------------------------

def test_pfm_to_png_display_option(tmp_path):
    """tools/pfm_to_png.py IN OUT --display key=value sends the PFM through the CPU twin; without the option the
    output is the clamp-and-sqrt picture it always was."""
    import os
    import subprocess
    import sys
    from PIL import Image
    acc = frame("b")
    h, w = acc.shape[:2]
    mean = np.ones_like(acc)
    mean[..., :3] = acc[..., :3] / acc[..., 3:]
    src = str(tmp_path / "in.pfm")
    assert surf_amd.load().surf_write_pfm(src.encode(), w, h, mean.ctypes.data) == 0
    tool = os.path.join(surf_amd.REPO_ROOT, "tools", "pfm_to_png.py")
    rgb = lambda path: np.asarray(Image.open(path).convert("RGB")).astype(np.uint32)
    run = subprocess.run([sys.executable, tool, src, str(tmp_path / "d.png"), "--display", "bloom_radius=4", "bloom_threshold=0.5"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    want, meter, _ = np_display(mean, bloom_radius=4, bloom_threshold=0.5)
    got = rgb(tmp_path / "d.png")
    assert np.array_equal(got[..., 0] | got[..., 1] << 8 | got[..., 2] << 16, want & 0xFFFFFF)
    assert f"median bin {meter['median_bin']}" in run.stdout
    run = subprocess.run([sys.executable, tool, src, str(tmp_path / "p.png")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    plain = (np.sqrt(np.clip(mean[..., :3], 0.0, 1.0)) * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(rgb(tmp_path / "p.png"), plain)
