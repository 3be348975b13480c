"""The mask from the non-local-means filter's error estimate and the adaptive loop on it
(surf_error_mask_image*, surf_mask_from_nlm, surf_render_adaptive_nlm; include/surf_hip.h) where
they need no GPU: exported symbols and defaults, status codes, the CPU twin against a numpy
restatement, the branches the inputs reach, the loop's restatement on the oracle's frames, and
the loop's error against uniform sampling.  CPU only.

Bar: bit-exact -- masks, lists and counts as integers.  The expected values never come from the
code under test: np_error_mask and np_adaptive_nlm below restate the header's rules on what the
suite already has -- np_nlm, np_buckets(..., active=), np_halves, oracle_samples, np_adaptive.

tests/test_gpu_nlm_adaptive.py imports the restatements, the cases and the loop's case from here.
"""
import ctypes as C
import math

import numpy as np
import pytest

import surf_amd
from test_adaptive_host import np_adaptive
from test_nlm_host import PLANTED as NLM_PLANTED, expected as nlm_expected, frame as nlm_frame, halves, np_nlm
from test_robust_host import np_buckets, np_halves, oracle_buckets, reference
from test_sampled_host import H, W, oracle_samples

F = np.float32
SURF_ERR_INVALID = -1
MASK_DEFAULTS = dict(threshold=0.1, floor=0.01, min_samples=16, max_samples=1024, smooth=3, dilate=1)
NLM_SMALL = dict(search_radius=3, patch_radius=1)
# the loop's case (the issue's): 100 x 37, M = 2, r 3, f 1, at least 4 and at most 36 samples, rounds of 4
LOOP = dict(threshold=0.12, floor=0.01, min_samples=4, max_samples=36, smooth=1, dilate=1, batch=4, **NLM_SMALL)
LOOP_M = 2


def error_key(S):
    """The header's order-preserving key of float32 values, as uint32."""
    b = np.asarray(S, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def np_error_mask(out, err, acc, **params):
    """The header's rule on three (H, W, 4) planes: (mask (H, W) uint8, ascending list of active indices, raw flags, S)."""
    p = {**MASK_DEFAULTS, **params}
    assert set(params) <= set(MASK_DEFAULTS)
    O, E, A = (np.asarray(v, np.float32) for v in (out, err, acc))
    h, w = A.shape[:2]
    tt, ff = F(p["threshold"]) * F(p["threshold"]), F(p["floor"]) * F(p["floor"])
    s, d = int(p["smooth"]), int(p["dilate"])
    ys, xs = np.arange(h), np.arange(w)
    with np.errstate(all="ignore"):
        num = (E[..., 0] + E[..., 1]) + E[..., 2]
        den = (((O[..., 0] * O[..., 0]) + (O[..., 1] * O[..., 1])) + (O[..., 2] * O[..., 2])) + ff
        rel = num / den
        assert rel.dtype == np.float32
        if s == 0:
            S = rel
        else:
            total = np.zeros((h, w), np.float32)
            for j in range(-s, s + 1):                                      # rows first ...
                row = np.zeros((h, w), np.float32)
                for i in range(-s, s + 1):
                    row = row + rel[np.clip(ys + j, 0, h - 1)][:, np.clip(xs + i, 0, w - 1)]
                total = total + row                                          # ... then the column of row sums
            S = total / F((2 * s + 1) * (2 * s + 1))
        assert S.dtype == np.float32
        n = A[..., 3]
        raw = ~(n >= F(p["min_samples"])) | ~(S <= tt)
    anyraw = np.zeros((h, w), bool)
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            yy, xx = ys + dy, xs + dx
            inside = ((yy >= 0) & (yy < h))[:, None] & ((xx >= 0) & (xx < w))[None, :]
            anyraw |= inside & raw[np.clip(yy, 0, h - 1)][:, np.clip(xx, 0, w - 1)]
    active = anyraw & (n < F(p["max_samples"]))
    return active.astype(np.uint8), np.flatnonzero(active).astype(np.uint32), raw, S


def np_error_summary(acc, S, **params):
    """The loop's summary of a final state: (above, max_error as float32)."""
    p = {**MASK_DEFAULTS, **params}
    tt = F(p["threshold"]) * F(p["threshold"])
    with np.errstate(all="ignore"):
        above = int(((acc[..., 3] >= F(p["min_samples"])) & ~(S <= tt)).sum())
    good = S[~np.isnan(S)]
    if good.size == 0:
        return above, F(0.0)
    best = good[np.argmax(error_key(good))]
    return above, F(best)


def np_adaptive_nlm(samples, M, first=0, **params):
    """The loop's definition on per-sample frames (samples[j] = the frame of sample index j) through M buckets."""
    p = {**MASK_DEFAULTS, "batch": 64, "search_radius": 5, "patch_radius": 2, **params}
    mp = {k: p[k] for k in MASK_DEFAULTS}
    fp = {k: p[k] for k in p if k not in MASK_DEFAULTS and k != "batch"}
    h, w = samples[0].shape[:2]
    A, B = np_buckets(samples[first:first + p["min_samples"]], M)
    f, total = p["min_samples"], p["min_samples"] * h * w
    round_active, rounds = [], []
    while True:
        h0, h1 = np_halves(B)
        out, err, _ = np_nlm(h0, h1, **fp)
        mask, lst, raw, S = np_error_mask(out, err, A, **mp)
        rounds.append({"out": out, "err": err, "acc": A, "mask": mask, "list": lst, "raw": raw})
        if len(lst) == 0 or f == p["max_samples"]:
            break
        nb = min(p["batch"], p["max_samples"] - f)
        round_active.append(len(lst))
        A, B = np_buckets(samples[first + f:first + f + nb], M, A, B, active=mask)
        total += nb * len(lst)
        f += nb
    above, max_error = np_error_summary(A, S, **mp)
    return {"acc": A, "buckets": B, "mask": mask, "image": out, "err": err, "S": S, "states": rounds, "round_active": round_active,
            "rounds": len(round_active), "frames": f, "samples": total, "active_last": int(mask.sum()), "above": above, "max_error": max_error}


_loop = {}


def loop_case():
    """np_adaptive_nlm of the oracle's first 36 frames at 100 x 37 under LOOP; computed once, read only."""
    if not _loop:
        samples, _, _ = oracle_samples(LOOP["max_samples"])
        _loop["want"] = np_adaptive_nlm(samples, LOOP_M, **LOOP)
    return _loop["want"]


# ---- the frames ---------------------------------------------------------------------------------

_frames = {}
PLANT_MIN, PLANT_MAX = 4, 8          # the planted frame holds 6 samples per pixel: between the two
PLANT = {"nan": (6, 5), "inf": (3, 27), "below": (7, 14), "at_max": (1, 30), "past_max": (5, 2)}


def filtered(count, w, h, M=2):
    """(out, err, acc) of the oracle's first `count` samples at w x h: np_nlm at r 3, f 1 of the halves; computed once."""
    key = (count, w, h, M)
    if key not in _frames:
        h0, h1 = halves(count, w, h, M)
        out, err, _ = np_nlm(h0, h1, **NLM_SMALL)
        acc = np_buckets(oracle_samples(count, w, h)[0], M)[0]
        for a in (out, err, acc):
            a.setflags(write=False)
        _frames[key] = (out, err, acc)
    return _frames[key]


def frame_a():
    """100 x 37, 16 samples; the filter's output is test_nlm_host's."""
    if "a" not in _frames:
        out, err, _ = nlm_expected("a", (3, 1))
        _frames["a"] = (out, err, oracle_buckets(16, 2)[0])
    return _frames["a"]


def frame_planted():
    """test_nlm_host's planted 33 x 9 frame (6 samples; three pixels the filter marks invalid, whose err is 0) through
    the filter, then: a NaN and an Inf in err, a pixel below min_samples, one at and one past max_samples."""
    out, err, _ = nlm_expected("planted", (3, 1))
    h0, h1 = nlm_frame("planted")
    out, err = out.copy(), err.copy()
    acc = (h0 + h1).astype(np.float32)
    acc[NLM_PLANTED["empty"]][3] = 6.0              # the invalid pixels have their samples: only err = 0 speaks for them
    err[PLANT["nan"]][1] = np.nan
    err[PLANT["inf"]][0] = np.inf
    acc[PLANT["below"]][3] = 3.0
    acc[PLANT["at_max"]][3] = 8.0
    acc[PLANT["past_max"]][3] = 9.0
    return out, err, acc


def frame_corners():
    """The 33 x 9 frame of 6 samples with a huge err in each corner pixel: under a threshold nothing else exceeds,
    the only noisy pixels."""
    out, err, acc = (a.copy() for a in filtered(6, 33, 9, 4))
    for y in (0, 8):
        for x in (0, 32):
            err[y, x, :3] = 1e20
    return out, err, acc


CORNER_THRESHOLD = 1e3


def error_threshold(out, err, acc, smooth):
    """A threshold about half of the pixels exceed: the root of the median S."""
    S = np_error_mask(out, err, acc, smooth=smooth)[3]
    return float(np.sqrt(np.median(S[np.isfinite(S) & (S > 0)])))


def mask_cases():
    """(name, out, err, acc, params) of every frame the mask rule is checked on."""
    cases = []
    frames = {"100x37": frame_a(), "70x1": filtered(4, 70, 1), "1x40": filtered(4, 1, 40), "1x1": filtered(4, 1, 1)}
    for name, (out, err, acc) in frames.items():
        n = int(acc[0, 0, 3])
        for s in (0, 1, 2, 3):
            for d in (0, 1, 2):
                if name != "100x37" and (s, d) not in ((0, 0), (1, 1), (3, 2)):
                    continue
                thr = error_threshold(out, err, acc, s) if name != "1x1" else 1e-3
                cases.append((f"{name} smooth {s} dilate {d}", out, err, acc, dict(threshold=thr, min_samples=2, max_samples=n + 1, smooth=s, dilate=d)))
        cases.append((f"{name} below min_samples", out, err, acc, dict(min_samples=n + 1, max_samples=n + 2)))
        cases.append((f"{name} at max_samples", out, err, acc, dict(threshold=1e-6, min_samples=2, max_samples=n)))
    out, err, acc = frame_planted()
    thr = error_threshold(*filtered(6, 33, 9, 4), 0)
    for s, d in ((0, 0), (0, 1), (1, 0), (2, 1), (3, 2)):
        cases.append((f"planted smooth {s} dilate {d}", out, err, acc, dict(threshold=thr, min_samples=PLANT_MIN, max_samples=PLANT_MAX, smooth=s, dilate=d)))
        cases.append((f"planted quiet smooth {s} dilate {d}", out, err, acc,
                      dict(threshold=1e6, min_samples=PLANT_MIN, max_samples=PLANT_MAX, smooth=s, dilate=d)))
    out, err, acc = frame_corners()
    for s in (0, 1, 2, 3):
        for d in (0, 1, 2):
            cases.append((f"corners smooth {s} dilate {d}", out, err, acc,
                          dict(threshold=CORNER_THRESHOLD, min_samples=PLANT_MIN, max_samples=PLANT_MAX, smooth=s, dilate=d)))
    return cases


def check_error_mask(fn, what, cases=None):
    """fn(out, err, acc, **params) -> (mask, list) against np_error_mask on every case."""
    for name, out, err, acc, params in (mask_cases() if cases is None else cases):
        want_mask, want_list, _, _ = np_error_mask(out, err, acc, **params)
        mask, lst = fn(out, err, acc, **params)
        assert mask.dtype == np.uint8 and mask.shape == want_mask.shape, (what, name)
        assert np.array_equal(mask, want_mask), (what, name, int((mask != want_mask).sum()))
        assert len(lst) == len(want_list) and np.array_equal(lst, want_list), (what, name)
        assert np.all(np.diff(lst.astype(np.int64)) > 0) and np.array_equal(lst, np.flatnonzero(mask)), (what, name)


# ---- 1. symbols, defaults, checks --------------------------------------------------------------

NEW_SYMBOLS = ("surf_error_mask_default_params", "surf_error_mask_image", "surf_error_mask_image_host", "surf_mask_from_nlm",
               "surf_debug_error_mask_time", "surf_adaptive_nlm_default_params", "surf_render_adaptive_nlm",
               "surf_render_adaptive_nlm_copy_device")


def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("ErrorMaskParams", "AdaptiveNlmParams", "AdaptiveNlmSummary", "error_mask_params", "adaptive_nlm_params", "error_mask_image_host"):
        assert hasattr(surf_amd, name), name
    for name in ("error_mask_image", "mask_from_nlm", "render_adaptive_nlm", "debug_error_mask_time"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_params():
    lib = surf_amd.load()
    p = surf_amd.ErrorMaskParams()
    assert C.sizeof(p) == 32 and C.sizeof(surf_amd.AdaptiveNlmParams) == 72 and C.sizeof(surf_amd.AdaptiveNlmSummary) == 40
    p.smooth, p._pad[1] = 9, 7
    assert lib.surf_error_mask_default_params(C.byref(p)) == 0
    got = dict(threshold=p.threshold, floor=p.floor, min_samples=p.min_samples, max_samples=p.max_samples, smooth=p.smooth, dilate=p.dilate)
    assert got == {k: (F(v) if isinstance(v, float) else v) for k, v in MASK_DEFAULTS.items()} and p._pad[1] == 0
    a = surf_amd.AdaptiveNlmParams()
    assert lib.surf_adaptive_nlm_default_params(C.byref(a)) == 0
    assert (F(a.mask.threshold), a.mask.min_samples, a.mask.max_samples, a.mask.smooth, a.mask.dilate) == (F(MASK_DEFAULTS["threshold"]), 16, 1024,
                                                                                                             MASK_DEFAULTS["smooth"], 1)
    assert (a.nlm.search_radius, a.nlm.patch_radius, F(a.nlm.k), F(a.nlm.alpha), F(a.nlm.eps)) == (5, 2, F(0.45), F(1.0), F(1e-10))
    assert (a.batch, a.max_segments, a.first_sample_index) == (64, 0, 0)
    assert lib.surf_error_mask_default_params(None) == SURF_ERR_INVALID
    assert lib.surf_adaptive_nlm_default_params(None) == SURF_ERR_INVALID
    q = surf_amd.adaptive_nlm_params(smooth=1, search_radius=3, batch=4)
    assert (q.mask.smooth, q.nlm.search_radius, q.nlm.patch_radius, q.batch) == (1, 3, 2, 4)
    with pytest.raises(TypeError):
        surf_amd.error_mask_params(sigma=1.0)
    with pytest.raises(TypeError):
        surf_amd.adaptive_nlm_params(sigma=1.0)


def test_invalid_arguments_are_status_codes():
    lib = surf_amd.load()
    out, err, acc = (np.ascontiguousarray(a) for a in filtered(6, 33, 9, 4))
    h, w = acc.shape[:2]
    mask, lst, n = np.zeros((h, w), np.uint8), np.zeros(h * w, np.uint32), C.c_uint32()
    host = lib.surf_error_mask_image_host
    good = surf_amd.error_mask_params()

    def call(p=good, ww=w, hh=h, o=out.ctypes.data, e=err.ctypes.data, a=acc.ctypes.data, m=mask.ctypes.data, l=lst.ctypes.data, cnt=C.byref(n)):
        return host(ww, hh, o, e, a, C.byref(p) if p is not None else None, m, l, cnt)

    assert call() == 0
    assert call(l=None) == 0                                                               # the list is optional
    for kw in (dict(o=None), dict(e=None), dict(a=None), dict(m=None), dict(cnt=None), dict(p=None), dict(ww=0), dict(hh=0)):
        assert call(**kw) == SURF_ERR_INVALID, kw
    nan, inf = float("nan"), float("inf")
    bad = {"threshold": (0.0, -1.0, nan, inf), "floor": (0.0, -1.0, nan, inf), "min_samples": (0, 1), "smooth": (4, 0xFFFFFFFF),
           "dilate": (3, 0xFFFFFFFF)}
    for field, values in bad.items():
        for v in values:
            assert call(p=surf_amd.error_mask_params(**{field: v})) == SURF_ERR_INVALID, (field, v)
    assert call(p=surf_amd.error_mask_params(min_samples=8, max_samples=7)) == SURF_ERR_INVALID
    for ok in (dict(min_samples=2, max_samples=2), dict(smooth=0), dict(smooth=3), dict(dilate=0), dict(dilate=2), dict(threshold=1e-6), dict(floor=1e3)):
        assert call(p=surf_amd.error_mask_params(**ok)) == 0, ok
    with pytest.raises(surf_amd.SurfError) as ex:
        surf_amd.error_mask_image_host(out, err, acc, smooth=4)
    assert ex.value.code == SURF_ERR_INVALID and "smooth" in str(ex.value)
    with pytest.raises(ValueError):
        surf_amd.error_mask_image_host(out, err[:, :5], acc)
    # a NULL context
    ms = (C.c_float * 2)()
    s, ap, fp = surf_amd.AdaptiveNlmSummary(), surf_amd.adaptive_nlm_params(), surf_amd.nlm_params()
    o, e, a, m = out.ctypes.data, err.ctypes.data, acc.ctypes.data, mask.ctypes.data
    assert lib.surf_error_mask_image(None, w, h, o, e, a, C.byref(good), m, None, C.byref(n)) == SURF_ERR_INVALID
    assert lib.surf_mask_from_nlm(None, C.byref(fp), C.byref(good), C.byref(n)) == SURF_ERR_INVALID
    assert lib.surf_debug_error_mask_time(None, ms, 2) == SURF_ERR_INVALID
    assert lib.surf_render_adaptive_nlm(None, C.byref(ap), o, e, None, 0, C.byref(s)) == SURF_ERR_INVALID
    assert lib.surf_render_adaptive_nlm_copy_device(None, C.byref(ap), None, None, None, 0, C.byref(s)) == SURF_ERR_INVALID


# ---- 2. the mask rule --------------------------------------------------------------------------

def test_mask_host_matches_numpy():
    check_error_mask(surf_amd.error_mask_image_host, "host twin")


def test_cases_reach_the_branches():
    """What the frames above are for, stated on the numpy side."""
    out, err, acc = frame_planted()
    thr = error_threshold(*filtered(6, 33, 9, 4), 0)
    p = dict(threshold=thr, min_samples=PLANT_MIN, max_samples=PLANT_MAX)
    mask0, _, raw, S = np_error_mask(out, err, acc, smooth=0, dilate=0, **p)
    for k in ("empty", "nan", "inf"):                                                             # the filter's invalid pixels: err = 0 ...
        assert not err[NLM_PLANTED[k]].any(), k
    e = NLM_PLANTED["empty"]
    assert S[e] == 0 and acc[e][3] >= PLANT_MIN and not raw[e] and not mask0[e]                   # ... so quiet once past min_samples
    assert np.isnan(S[NLM_PLANTED["nan"]]) and raw[NLM_PLANTED["nan"]]                             # (its out holds a NaN: den is NaN, noisy)
    assert np.isnan(S[PLANT["nan"]]) and raw[PLANT["nan"]] and mask0[PLANT["nan"]]                 # a NaN in err counts as noisy
    assert np.isinf(S[PLANT["inf"]]) and raw[PLANT["inf"]] and mask0[PLANT["inf"]]
    quiet = np_error_mask(out, err, acc, smooth=0, dilate=0, **{**p, "threshold": 1e6})
    assert quiet[2][PLANT["below"]] and quiet[0][PLANT["below"]]                                   # below min_samples: active whatever S is
    assert quiet[2][PLANT["nan"]] and quiet[2][PLANT["inf"]] and not quiet[2][e]
    loud = np_error_mask(out, err, acc, smooth=0, dilate=2, **{**p, "threshold": 1e-6})
    assert loud[2][PLANT["at_max"]] and not loud[0][PLANT["at_max"]] and not loud[0][PLANT["past_max"]]   # at the cap: never active
    assert 0 < mask0.sum() < mask0.size and 0 < raw.sum() < raw.size
    smoothed = np_error_mask(out, err, acc, smooth=1, dilate=0, **p)[3]
    y, x = PLANT["nan"]
    assert np.isnan(smoothed[y - 1:y + 2, x - 1:x + 2]).all() and not np.isnan(smoothed[y, x + 2])   # the box spreads a NaN over 3 x 3
    # the corners: clamped smoothing and in-frame dilation
    out, err, acc = frame_corners()
    cp = dict(threshold=CORNER_THRESHOLD, min_samples=PLANT_MIN, max_samples=PLANT_MAX)
    for d, count in ((0, 4), (1, 16), (2, 36)):                                                    # the dilation clipped at each corner
        mask, lst, raw, _ = np_error_mask(out, err, acc, smooth=0, dilate=d, **cp)
        assert raw.sum() == 4 and raw[0, 0] and raw[0, 32] and raw[8, 0] and raw[8, 32] and mask.sum() == count, d
        assert lst[0] == 0 and lst[-1] == 33 * 9 - 1
    for s in (1, 2, 3):
        mask, _, raw, S = np_error_mask(out, err, acc, smooth=s, dilate=0, **cp)
        assert raw.sum() == 4 * (s + 1) ** 2, s                                                    # the pixels whose box reaches a corner
        # the clamped window holds the corner texel (s + 1)^2 times at the corner, once at distance s
        assert S[0, 0] > F(0.9) * F((s + 1) ** 2) * S[s, s] and S[s, s] > 0 and S[8, 32] > F(0.9) * F((s + 1) ** 2) * S[8 - s, 32 - s]
    # one row, one column, one pixel: every border clips
    for shape in ((70, 1), (1, 40), (1, 1)):
        out, err, acc = filtered(4, *shape)
        assert np_error_mask(out, err, acc, min_samples=5, max_samples=6, smooth=3, dilate=2)[0].all()


# ---- 3. the loop's restatement on the oracle's frames -------------------------------------------

def test_loop_restatement_conditions():
    """The loop's case does what it is chosen for: at least two rounds, every round's active count strictly between 0
    and W * H, some pixel stopped before max_samples.  The threshold 0.12 was chosen on the CPU from np_adaptive_nlm
    for these conditions (they are conditions, not measurements); it observes eight rounds of 3584, 3325, 2943, 2705,
    2300, 2060, 1954 and 1817 active pixels of 3700, 97552 samples of 133200, 39 pixels left at 4 samples, 1307 at 36,
    834 above the threshold at the end, max_error 0.35011077.  The host twin is checked on every round's planes."""
    want = loop_case()
    counts = want["acc"][..., 3]
    values = np.unique(counts)
    print("final counts:", {int(v): int((counts == v).sum()) for v in values}, "samples", want["samples"], "rounds", want["round_active"],
          "above", want["above"], "max_error", want["max_error"])
    assert want["rounds"] >= 2 and len(want["round_active"]) == want["rounds"]
    assert all(0 < n < W * H for n in want["round_active"])
    assert (counts < LOOP["max_samples"]).any() and (counts == LOOP["min_samples"]).any()
    assert want["samples"] == int(counts.sum()) and want["samples"] < LOOP["max_samples"] * W * H
    assert want["frames"] == LOOP["min_samples"] + LOOP["batch"] * want["rounds"]
    b = want["buckets"][..., 3]
    assert np.array_equal(b.sum(0), counts) and (np.abs(b[0] - b[1]) <= 1).all()              # the buckets stay balanced under the masks
    mp = {k: LOOP[k] for k in MASK_DEFAULTS}
    for r, st in enumerate(want["states"]):
        mask, lst = surf_amd.error_mask_image_host(st["out"], st["err"], st["acc"], **mp)
        assert np.array_equal(mask, st["mask"]) and np.array_equal(lst, st["list"]), r
    again = np.zeros(counts.shape, bool)
    stopped = np.zeros(counts.shape, bool)
    for st in want["states"]:
        again |= stopped & (st["mask"] != 0)
        stopped |= st["mask"] == 0
    assert again.any()                                                                          # a stopped pixel can come back


# ---- 4. quality ------------------------------------------------------------------------------------

QUALITY = dict(threshold=0.1, floor=0.01, min_samples=16, max_samples=64, smooth=3, dilate=1, batch=16)   # the library's mask defaults
QUALITY_NOISE = dict(threshold=0.45, floor=0.01, min_samples=16, max_samples=64, dilate=1, batch=16)
RATIO_UNIFORM = 1.13     # np_adaptive_nlm measures 0.9775 against uniform sampling; x 1.15, rounded up to two decimals


def replay_buckets(samples, M, state, **params):
    """The buckets of a noise-driven np_adaptive run: its rounds' frames added again under its masks."""
    A, B = np_buckets(samples[:params["min_samples"]], M)
    f = params["min_samples"]
    for mask in state["masks"][:state["rounds"]]:
        nb = min(params["batch"], params["max_samples"] - f)
        A, B = np_buckets(samples[f:f + nb], M, A, B, active=mask)
        f += nb
    assert np.array_equal(A[..., 3], state["acc"][..., 3])
    return A, B


def test_loop_against_uniform_sampling():
    """The oracle's indoor scene at 100 x 37, spp-1 frames from frame 0 through two buckets, the filter's default
    parameters, mean absolute error over all pixels against the oracle's 2048-spp render of the same view
    (first_frame 100000), set up as test_nlm_host's quality test: the loop's final image (np_adaptive_nlm at the
    library's mask defaults, min_samples 16, max_samples 64, batch 16) against np_nlm of a uniform render whose
    per-pixel count is the loop's mean sample count rounded UP -- both restatements, never the library.  The
    noise-driven loop (np_adaptive, threshold 0.45: the nearest budget on a 0.01 grid) through the same filter is
    printed, not asserted.  The asserted ratio is the measured one x 1.15, rounded up to two decimals
    (test_sampled_host's RATIO_64 convention; the margin is for retuning, the result is deterministic).
    np_adaptive_nlm measures (MEASUREMENTS "Error-driven adaptive sampling"), mean samples per pixel, the loop's MAE /
    uniform sampling's at the count rounded up, ratio:
    smooth 3, threshold 0.1   34.46   0.01127 / 0.01153 (35 samples)   0.9775, asserted <= 1.13
    and over smooth 0..3 x threshold 0.05, 0.1, 0.15, 0.2 ratios from 0.9707 to 1.0240: the loop is level with
    uniform sampling on this scene, not clearly ahead of it -- two 8192-spp references differ by an MAE of 0.008
    (test_robust_host), which a difference of 2 % of 0.011 is far inside.  smooth 3 is the one radius whose ratio is
    below 1 at all four thresholds; threshold 0.1 stops about half of the pixels before the cap."""
    samples, _, _ = oracle_samples(QUALITY["max_samples"])
    ref = reference()
    mae = lambda img: float(np.abs(img[..., :3].astype(np.float64) - ref).mean())
    want = np_adaptive_nlm(samples, 2, **QUALITY)
    mean = want["samples"] / (W * H)
    n = math.ceil(mean)
    loop, uniform = mae(want["image"]), mae(np_nlm(*halves(n))[0])
    print(f"error-driven: rounds {want['round_active']}, mean samples {mean:.2f}, MAE {loop:.5f}; uniform at {n}: {uniform:.5f}; "
          f"ratio {loop / uniform:.4f}; above {want['above']}, max_error {want['max_error']}")
    noise = np_adaptive(samples, **QUALITY_NOISE)
    _, B = replay_buckets(samples, 2, noise, **QUALITY_NOISE)
    driven = mae(np_nlm(*np_halves(B))[0])
    nmean = noise["samples"] / (W * H)
    print(f"noise-driven: rounds {noise['round_active']}, mean samples {nmean:.2f}, MAE {driven:.5f}; "
          f"ratio to uniform at {math.ceil(nmean)}: {driven / mae(np_nlm(*halves(math.ceil(nmean)))[0]):.4f}")
    mask, lst = surf_amd.error_mask_image_host(want["image"], want["err"], want["acc"], **{k: QUALITY[k] for k in MASK_DEFAULTS})
    assert np.array_equal(mask, want["mask"]) and np.array_equal(lst, np.flatnonzero(want["mask"]))
    assert 0 < want["rounds"] and mean < QUALITY["max_samples"]
    assert loop / uniform <= RATIO_UNIFORM, (loop / uniform, loop, uniform)
