"""Per-pixel sample masks and the adaptive loop (surf_set_pixel_mask, surf_mask_from_noise,
surf_adaptive_mask_image*, surf_render_adaptive, surf_*_rgba8_weighted; include/surf_hip.h)
where they need no GPU: exported symbols and defaults, parameter checks, the CPU twins
against numpy restatements, and the loop's restatement on the oracle's frames.  CPU only.

Bar: bit-exact -- masks and lists as integers, packed images as uint32 words.  The expected
values never come from the code under test: np_mask, np_pack_weighted and np_adaptive below
restate the header's arithmetic on the oracle's spp-1 frames (oracle_samples), summed by
np_squares, with np_noise's error.

tests/test_gpu_adaptive.py imports the restatements and the frames from here.
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from test_sampled_host import W, H, frame_a, frame_b, lum, noise_threshold, np_noise, np_squares, oracle_samples

F = np.float32
SURF_ERR_INVALID = -1
MASK_DEFAULTS = dict(threshold=0.05, floor=0.01, min_samples=16, max_samples=1024, dilate=1)
# the loop's case (the issue's): 100 x 37, at least 4 and at most 36 samples, rounds of 4
LOOP = dict(threshold=0.5, floor=0.01, min_samples=4, max_samples=36, dilate=1, batch=4)


def np_mask(acc, squares, **params):
    """The header's rule: (mask (H, W) uint8, ascending list of active indices, raw flags)."""
    p = {**MASK_DEFAULTS, **params}
    assert set(params) <= set(MASK_DEFAULTS)
    A, Q = np.asarray(acc, np.float32), np.asarray(squares, np.float32)
    h, w = A.shape[:2]
    e, _ = np_noise(A, Q, p["threshold"], p["floor"])
    n = A[..., 3]
    with np.errstate(all="ignore"):
        raw = ~(n >= F(p["min_samples"])) | ~(e <= F(p["threshold"]))
    d = p["dilate"]
    anyraw = np.zeros((h, w), bool)
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            ys, xs = np.arange(h) + dy, np.arange(w) + dx
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            anyraw |= inside & raw[np.clip(ys, 0, h - 1)][:, np.clip(xs, 0, w - 1)]
    active = anyraw & (n < F(p["max_samples"]))
    return active.astype(np.uint8), np.flatnonzero(active).astype(np.uint32), raw


def np_pack_weighted(acc, display=False):
    """The header's weighted packing of (..., 4) records, as uint32 words."""
    A = np.asarray(acc, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        inv = np.where(A[:, 3] > F(0.0), F(1.0) / A[:, 3], F(0.0)).astype(np.float32)
        v = (A * inv[:, None]) * F(255.0)
        assert v.dtype == np.float32
        ok = (v >= F(-2147483648.0)) & (v < F(2147483648.0))
        r = np.rint(np.where(ok, v, F(0.0)))                       # round half to even, as rintf
        c = np.where(ok, np.clip(r, 0.0, 255.0), 0.0).astype(np.uint32)
        if display:
            s = np.sqrt(c.astype(np.float32) / F(255.0)) * F(255.0)
            assert s.dtype == np.float32
            c = np.clip(np.rint(s), 0.0, 255.0).astype(np.uint32)
    return c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)


def np_add_frame(A, Q, r, mask):
    """One spp-1 frame added to the records of the mask's pixels, as np_squares adds it."""
    r = np.asarray(r, np.float32)
    l = lum(r)
    q = np.stack([r[..., 0] * r[..., 0], r[..., 1] * r[..., 1], r[..., 2] * r[..., 2], l * l], -1)
    m = mask.astype(bool)[..., None]
    A, Q = np.where(m, A + r, A), np.where(m, Q + q, Q)
    assert A.dtype == np.float32 and Q.dtype == np.float32
    return A, Q


def np_adaptive(samples, first=0, **params):
    """The loop's definition on per-sample frames (samples[j] = the frame of sample index j)."""
    p = {**MASK_DEFAULTS, "batch": 64, **params}
    mp = {k: p[k] for k in MASK_DEFAULTS}
    h, w = samples[0].shape[:2]
    A, Q = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    every = np.ones((h, w), np.uint8)
    for j in range(p["min_samples"]):
        A, Q = np_add_frame(A, Q, samples[first + j], every)
    f, total = p["min_samples"], p["min_samples"] * h * w
    round_active, masks, raws = [], [], []
    while True:
        mask, lst, raw = np_mask(A, Q, **mp)
        masks.append(mask)
        raws.append(raw)
        if len(lst) == 0 or f == p["max_samples"]:
            break
        nb = min(p["batch"], p["max_samples"] - f)
        round_active.append(len(lst))
        for j in range(nb):
            A, Q = np_add_frame(A, Q, samples[first + f + j], mask)
        total += nb * len(lst)
        f += nb
    _, noise = np_noise(A, Q, p["threshold"], p["floor"])
    return {"acc": A, "squares": Q, "mask": masks[-1], "masks": masks, "raws": raws, "round_active": round_active, "rounds": len(round_active),
            "frames": f, "samples": total, "active_last": int(masks[-1].sum()), "noise": noise}


_loop = {}


def loop_case():
    """np_adaptive of the oracle's first 36 frames at 100 x 37 under LOOP; computed once, read only."""
    if not _loop:
        samples, _, _ = oracle_samples(LOOP["max_samples"])
        _loop["want"] = np_adaptive(samples, **LOOP)
    return _loop["want"]


# ---- the frames ---------------------------------------------------------------------------------

PLANT_MIN, PLANT_MAX = 4, 8          # frame B holds 5 samples per pixel: between the two


def frame_planted():
    """Frame B (33 x 9, n = 5) with planted records: no sample, one sample, n at and past
    max_samples, NaN squares (t becomes 0: quiet), a NaN accumulator (e is NaN: noisy),
    squares too small for the mean (t < 0: quiet)."""
    A, Q, _, _ = frame_b()
    A, Q = A.copy(), Q.copy()
    A[2, 3], Q[2, 3] = 0.0, 0.0
    A[2, 8], Q[2, 8] = (0.25, 0.5, 0.125, 1.0), (0.0625, 0.25, 0.015625, 0.17)
    A[4, 15, 3] = 8.0
    A[4, 20, 3] = 9.0
    Q[6, 5, 3] = np.nan
    A[6, 12, 1] = np.nan
    Q[7, 25] = Q[7, 25] * F(0.001)
    return A, Q


def frame_corner():
    """Frame B with one sample in its last pixel: under a threshold nothing else exceeds, the
    lone raw pixel of the frame, in a corner."""
    A, Q, _, _ = frame_b()
    A, Q = A.copy(), Q.copy()
    A[8, 32], Q[8, 32] = (0.25, 0.5, 0.125, 1.0), (0.0625, 0.25, 0.015625, 0.17)
    return A, Q


def small_frame(w, h, count=5):
    samples, _, _ = oracle_samples(count, w, h)
    return np_squares(samples)


def mask_cases():
    """(name, A, Q, params) of every frame the mask rule is checked on."""
    cases = []
    for name, (A, Q) in {"33x9": frame_b()[:2], "100x37": frame_a()[:2], "1x1": small_frame(1, 1), "5x300": small_frame(5, 300)}.items():
        n = int(A[0, 0, 3])
        for d in (0, 1, 2):
            cases.append((f"{name} dilate {d}", A, Q, dict(threshold=noise_threshold(A, Q), min_samples=2, max_samples=n + 1, dilate=d)))
        cases.append((f"{name} below min_samples", A, Q, dict(min_samples=n + 1, max_samples=n + 2)))
        cases.append((f"{name} at max_samples", A, Q, dict(threshold=1e-6, min_samples=2, max_samples=n)))
    A, Q = frame_planted()
    for d in (0, 1, 2):
        cases.append((f"planted dilate {d}", A, Q, dict(threshold=noise_threshold(*frame_b()[:2]), min_samples=PLANT_MIN, max_samples=PLANT_MAX, dilate=d)))
        cases.append((f"planted quiet dilate {d}", A, Q, dict(threshold=1e6, min_samples=PLANT_MIN, max_samples=PLANT_MAX, dilate=d)))
    A, Q = frame_corner()
    for d in (0, 1, 2):
        cases.append((f"corner dilate {d}", A, Q, dict(threshold=1e6, min_samples=PLANT_MIN, max_samples=PLANT_MAX, dilate=d)))
    return cases


def check_mask(fn, what):
    """fn(A, Q, **params) -> (mask, list) against np_mask on every case."""
    for name, A, Q, params in mask_cases():
        want_mask, want_list, _ = np_mask(A, Q, **params)
        mask, lst = fn(A, Q, **params)
        assert mask.dtype == np.uint8 and mask.shape == want_mask.shape, (what, name)
        assert np.array_equal(mask, want_mask), (what, name, int((mask != want_mask).sum()))
        assert np.array_equal(lst, want_list), (what, name)
        assert np.all(np.diff(lst.astype(np.int64)) > 0) and np.array_equal(lst, np.flatnonzero(mask)), (what, name)


# ---- 1. symbols, defaults, checks --------------------------------------------------------------

NEW_SYMBOLS = ("surf_set_pixel_mask", "surf_get_pixel_mask", "surf_adaptive_default_mask_params", "surf_adaptive_default_params",
               "surf_mask_from_noise", "surf_adaptive_mask_image", "surf_adaptive_mask_image_host", "surf_render_adaptive",
               "surf_finalize_rgba8_weighted", "surf_pack_rgba8_weighted")


def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("AdaptiveMaskParams", "AdaptiveParams", "AdaptiveSummary", "adaptive_mask_image_host", "pack_rgba8_weighted"):
        assert hasattr(surf_amd, name), name
    for name in ("set_pixel_mask", "pixel_mask", "mask_from_noise", "render_adaptive", "finalize_weighted", "adaptive_mask_image"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_params():
    lib = surf_amd.load()
    p = surf_amd.AdaptiveMaskParams()
    assert C.sizeof(p) == 32 and C.sizeof(surf_amd.AdaptiveParams) == 48 and C.sizeof(surf_amd.AdaptiveSummary) == 48
    assert lib.surf_adaptive_default_mask_params(C.byref(p)) == 0
    assert (F(p.threshold), F(p.floor), p.min_samples, p.max_samples, p.dilate) == (F(0.05), F(0.01), 16, 1024, 1)
    a = surf_amd.AdaptiveParams()
    assert lib.surf_adaptive_default_params(C.byref(a)) == 0
    assert (F(a.mask.threshold), a.mask.min_samples, a.mask.max_samples, a.mask.dilate) == (F(0.05), 16, 1024, 1)
    assert (a.batch, a.max_segments, a.first_sample_index) == (64, 0, 0)
    assert lib.surf_adaptive_default_mask_params(None) == SURF_ERR_INVALID
    assert lib.surf_adaptive_default_params(None) == SURF_ERR_INVALID
    with pytest.raises(TypeError):
        surf_amd.adaptive_mask_params(sigma=1.0)


def test_parameter_checks():
    lib = surf_amd.load()
    A, Q, _, _ = frame_b()
    h, w = A.shape[:2]
    mask, lst, n = np.zeros((h, w), np.uint8), np.zeros(h * w, np.uint32), C.c_uint32()
    host = lib.surf_adaptive_mask_image_host
    good = surf_amd.adaptive_mask_params()

    def call(p=good, ww=w, hh=h, a=A.ctypes.data, q=Q.ctypes.data, m=mask.ctypes.data, l=lst.ctypes.data, cnt=C.byref(n)):
        return host(ww, hh, a, q, C.byref(p) if p is not None else None, m, l, cnt)

    assert call() == 0
    assert call(l=None) == 0                                                               # the list is optional
    for kw in (dict(a=None), dict(q=None), dict(m=None), dict(cnt=None), dict(p=None), dict(ww=0), dict(hh=0)):
        assert call(**kw) == SURF_ERR_INVALID, kw
    bad = {"threshold": (0.0, -1.0, float("nan"), float("inf")), "floor": (0.0, -1.0, float("nan"), float("inf")),
           "min_samples": (0, 1), "dilate": (3, 0xFFFFFFFF)}
    for field, values in bad.items():
        for v in values:
            assert call(p=surf_amd.adaptive_mask_params(**{field: v})) == SURF_ERR_INVALID, (field, v)
    assert call(p=surf_amd.adaptive_mask_params(min_samples=8, max_samples=7)) == SURF_ERR_INVALID
    for ok in (dict(min_samples=2, max_samples=2), dict(dilate=0), dict(dilate=2), dict(min_samples=8, max_samples=8)):
        assert call(p=surf_amd.adaptive_mask_params(**ok)) == 0, ok
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.adaptive_mask_image_host(A, Q, dilate=3)
    assert e.value.code == SURF_ERR_INVALID and "dilate" in str(e.value)
    # a NULL context
    s = surf_amd.AdaptiveSummary()
    ap = surf_amd.adaptive_params()
    assert lib.surf_set_pixel_mask(None, mask.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_get_pixel_mask(None, mask.ctypes.data, C.byref(n)) == SURF_ERR_INVALID
    assert lib.surf_mask_from_noise(None, C.byref(good), C.byref(n)) == SURF_ERR_INVALID
    assert lib.surf_adaptive_mask_image(None, w, h, A.ctypes.data, Q.ctypes.data, C.byref(good), mask.ctypes.data, None, C.byref(n)) == SURF_ERR_INVALID
    assert lib.surf_render_adaptive(None, C.byref(ap), None, 0, C.byref(s)) == SURF_ERR_INVALID
    assert lib.surf_finalize_rgba8_weighted(None, 0, lst.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_pack_rgba8_weighted(None, 1, 0, lst.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_pack_rgba8_weighted(A.ctypes.data, 1, 0, None) == SURF_ERR_INVALID


# ---- 2. the mask rule --------------------------------------------------------------------------

def test_mask_host_matches_numpy():
    check_mask(surf_amd.adaptive_mask_image_host, "host twin")


def test_cases_reach_the_branches():
    """What the frames above are for, stated on the numpy side."""
    A, Q = frame_planted()
    thr = noise_threshold(*frame_b()[:2])
    p = dict(threshold=thr, min_samples=PLANT_MIN, max_samples=PLANT_MAX)
    e, _ = np_noise(A, Q, thr, 0.01)
    mask0, _, raw = np_mask(A, Q, dilate=0, **p)
    assert raw[2, 3] and raw[2, 8] and e[2, 3] == F(1e30) and e[2, 8] == F(1e30)              # n = 0, n = 1
    assert not mask0[4, 15] and not mask0[4, 20]                                                 # n >= max_samples: never active
    assert e[6, 5] == 0 and e[7, 25] == 0 and not raw[6, 5] and not raw[7, 25]                   # NaN squares, t < 0: t = 0
    assert np.isnan(e[6, 12]) and raw[6, 12] and mask0[6, 12]                                    # a NaN error counts as noisy
    assert 0 < mask0.sum() < mask0.size and 0 < raw.sum() < raw.size                              # n = 5 on both sides
    mask1 = np_mask(A, Q, dilate=1, **p)[0]
    assert not mask1[4, 15] and not mask1[4, 20]
    quiet = np_mask(A, Q, dilate=1, **{**p, "threshold": 1e6})[0]
    assert quiet[1:4, 2:5].all() and quiet[1:4, 7:10].all() and quiet.sum() == 27               # 3 x 3 around n = 0, n = 1, the NaN
    A, Q = frame_corner()
    for d, count in ((0, 1), (1, 4), (2, 9)):                                                    # the dilation clipped at the corner
        mask, lst, raw = np_mask(A, Q, threshold=1e6, min_samples=PLANT_MIN, max_samples=PLANT_MAX, dilate=d)
        assert raw.sum() == 1 and raw[8, 32] and mask.sum() == count and lst[-1] == 33 * 9 - 1, d
    A, Q = small_frame(5, 300)
    assert np_mask(A, Q, min_samples=6, max_samples=7, dilate=2)[0].all()                         # every border clips, all active


# ---- 3. the weighted packing -------------------------------------------------------------------

def weighted_records():
    A, _ = frame_planted()                       # w = 0, 1, 5, 8, 9 and a NaN channel
    A = A.reshape(-1, 4).copy()
    extra = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 0.0], [4.0, 2.0, 1.0, 4.0], [1e30, -1.0, 0.5, 2.0], [np.inf, 0.00197, 0.00196, 1.0],
                      [0.5, 1.5, 2.5, 1.0], [2.0, 2.0, 2.0, -1.0]], np.float32)
    return np.concatenate([A, extra])


def test_pack_weighted_matches_numpy():
    A = weighted_records()
    assert (A[:, 3] == 0).any() and (A[:, 3] > 1).any()
    for display in (False, True):
        got = surf_amd.pack_rgba8_weighted(A, display)
        want = np_pack_weighted(A, display)
        assert got.dtype == np.uint32 and np.array_equal(got, want), (display, np.flatnonzero(got != want)[:8])
    assert surf_amd.pack_rgba8_weighted(A)[np.flatnonzero(A[:, 3] == 0)[0]] == 0                  # no sample: all four channels 0
    full = np.array([[2.0, 2.0, 2.0, 2.0]], np.float32)
    assert surf_amd.pack_rgba8_weighted(full)[0] == 0xFFFFFFFF                                   # alpha is w / w


# ---- 4. the loop's restatement on the oracle's frames -------------------------------------------

def test_loop_restatement_conditions():
    """The loop's case does what it is chosen for; checked on the numpy side alone."""
    want = loop_case()
    counts = want["acc"][..., 3]
    values = np.unique(counts)
    print("final counts:", {int(v): int((counts == v).sum()) for v in values}, "samples", want["samples"], "rounds", want["round_active"])
    assert len(values) >= 3
    assert (counts == LOOP["min_samples"]).any() and (counts == LOOP["max_samples"]).any()
    stopped = np.zeros(counts.shape, bool)
    again = np.zeros(counts.shape, bool)
    for m, raw in zip(want["masks"], want["raws"]):
        again |= stopped & (m != 0) & ~raw        # active again, quiet on its own account: a neighbour's flag brought it back
        stopped |= m == 0
    assert again.any()
    assert want["frames"] == LOOP["max_samples"] and want["rounds"] == (LOOP["max_samples"] - LOOP["min_samples"]) // LOOP["batch"]
    assert want["samples"] == int(counts.sum()) and want["samples"] < LOOP["max_samples"] * W * H
