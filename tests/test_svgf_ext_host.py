"""The variance-guided filter's two optional stages (surf_svgf_ext, include/surf_hip.h
"extensions"): the firefly clamp in front of the temporal accumulation and the
feedback of the first filtered iteration into the history -- where they need no
GPU: exported symbols, defaults and status codes, the CPU twins
(surf_firefly_image_host, surf_svgf_image_host_ex) against a numpy restatement,
the branches the fixtures reach, and what the stages do to the error against a
converged render.  CPU only.

Bar: bit-exact, images compared as uint32 words.  The expected images never
come from the code under test: np_firefly restates stage 0, every step an
explicit float32 numpy operation in the header's order, and np_svgf_ext puts it
in front of tests/test_svgf_host.py's np_svgf, which is called, not restated.
The fed-back history needs I_1: np_svgf with iterations=1 on the same inputs
returns (I_1.rgb * den, 1) for a valid pixel, which is the rule's colour.

tests/test_gpu_svgf_ext.py imports np_firefly, np_svgf_ext and the frames from here.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import surf_amd
from test_denoise_host import assert_images_equal
from test_svgf_host import albedo_of, assert_outputs_equal, lum, np_svgf, svgf_frames, with_moments  # noqa: F401
from test_temporal_host import CHAIN, W, H, frame_of, oracle_colour, temporal_frames  # noqa: F401

F = np.float32
SURF_ERR_INVALID = -1
EXTS = {"clamp": dict(firefly_scale=4.0), "feedback": dict(feedback=True), "both": dict(firefly_scale=4.0, feedback=True)}


def np_firefly(acc, albedo, scale, demodulate=1):
    """Stage 0 of the header.  Returns (A', counts)."""
    A, alb = np.asarray(acc, np.float32), np.asarray(albedo, np.float32)
    h, w = A.shape[:2]
    with np.errstate(all="ignore"):
        valid = alb[..., 3] != F(0.0)
        sampled = A[..., 3] > F(0.0)
        inv = np.where(sampled, F(1.0) / A[..., 3], F(0.0)).astype(np.float32)
        c = A[..., :3] * inv[..., None]
        a3 = alb[..., :3]
        den = np.where((valid & bool(demodulate))[..., None], np.where(a3 > F(0.01), a3, F(0.01)), F(1.0)).astype(np.float32)
        l = lum(c / den)
        assert l.dtype == np.float32
        usable = valid & sampled
        mx, cnt, skipped = np.zeros((h, w), np.float32), np.zeros((h, w), np.int32), 0
        ys0, xs0 = np.arange(h), np.arange(w)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                if dx == 0 and dy == 0:
                    continue
                ys, xs = ys0 + dy, xs0 + dx
                inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
                yc, xc = np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)
                use = inside & usable[yc][:, xc]
                skipped += int((inside & ~use).sum())
                lq = l[yc][:, xc]
                cnt = cnt + use
                mx = np.where(use & (lq > mx), lq, mx)
        lim = F(scale) * mx
        clamp = usable & (cnt > 0) & (l > lim)
        f = lim / l
        c2 = np.where(clamp[..., None], c * f[..., None], c)
        out = np.where(sampled[..., None], np.concatenate([c2, np.ones((h, w, 1), np.float32)], -1), F(0.0)).astype(np.float32)
    assert lim.dtype == np.float32 and f.dtype == np.float32
    counts = {"clamped": int(clamp.sum()), "unclamped": int((usable & (cnt > 0) & ~clamp).sum()), "invalid_centre": int((~valid).sum()),
              "unsampled_centre": int((~sampled).sum()), "skipped_neighbours": skipped, "cnt_zero": int((usable & (cnt == 0)).sum()),
              "nan_stays": int((usable & (cnt > 0) & np.isnan(l)).sum()), "energy": (float(lum(out[..., :3]).astype(np.float64).sum()),
                                                                                       float(lum(c).astype(np.float64).sum()))}
    return out, counts


def np_svgf_ext(cur, prev, firefly_scale=0.0, feedback=False, **params):
    """np_svgf with the two stages: (out, hist, moments, variance, counts)."""
    demod = params.get("demodulate", 1)
    if firefly_scale > 0.0:
        cur = {**cur, "acc": np_firefly(cur["acc"], cur["albedo"], firefly_scale, demod)[0]}
    out, hist, mom, var, cnt = np_svgf(cur, prev, **params)
    if feedback:
        first = np_svgf(cur, prev, **{**params, "iterations": 1})[0]
        valid = np.asarray(cur["albedo"], np.float32)[..., 3] != F(0.0)
        hist = hist.copy()
        hist[..., :3] = np.where(valid[..., None], first[..., :3], hist[..., :3])
        cnt = {**cnt, "fed_back": int(valid.sum()), "kept": int((~valid).sum())}
    return out, hist, mom, var, cnt


_chains = {}


def expected_ext_chain(frames, name, count, ext, **params):
    """[(out, hist, moments, variance, counts)] of np_svgf_ext along the first `count` frames of a
    list, the numpy history and moments fed forward; computed once."""
    key = (name, count, tuple(sorted(ext.items())), tuple(sorted(params.items())))
    if key not in _chains:
        res, prev = [], None
        for f in frames[name][:count]:
            r = np_svgf_ext(f, prev, **ext, **params)
            for a in r[:4]:
                a.setflags(write=False)
            res.append(r)
            prev = with_moments(f, r[1], r[2])
        _chains[key] = res
    return _chains[key]


# ---- the clamp's fixtures ---------------------------------------------------------------

@pytest.fixture(scope="session")
def firefly_fixtures(svgf_frames):
    """name -> (acc, albedo): 'real' the oracle's indoor frame 0 at 100 x 37 and 1 spp;
    'synthetic' the same with a block of invalid pixels, pixels without a sample -- one
    ring of them around a sampled pixel, which then has no usable neighbour -- and one
    NaN colour; 'one' a single pixel; 'tile' 33 x 9, seeded colour."""
    f0 = svgf_frames["a"][0]
    acc, alb = f0["acc"].copy(), f0["albedo"].copy()
    alb[10:16, 20:31, 3] = 0.0                       # invalid: centres, and neighbours of the block's rim
    acc[3, 70] = 0.0                                 # A.w == 0
    acc[0, 0] = 0.0                                  # ... in a corner
    acc[24:27, 49:52] = 0.0                          # a ring without samples ...
    acc[25, 50] = f0["acc"][25, 50]                  # ... around a sampled pixel: cnt == 0
    acc[30, 40, :3] = np.nan                         # a NaN colour, valid and sampled
    t0 = svgf_frames["tile"][0]
    fx = {"real": (f0["acc"], f0["albedo"]), "synthetic": (acc, alb),
          "one": (np.array([[[1.0, 2.0, 3.0, 1.0]]], np.float32), np.array([[[0.5, 0.5, 0.5, 1.0]]], np.float32)),
          "tile": (t0["acc"], t0["albedo"])}
    for pair in fx.values():
        for a in pair:
            a.setflags(write=False)
    return fx


# ---- 1. symbols, defaults, status codes ------------------------------------------------

def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in ("surf_svgf_default_ext", "surf_svgf_accumulate_ex", "surf_svgf_copy_device_ex", "surf_svgf_image_ex",
                 "surf_svgf_image_host_ex", "surf_firefly_image", "surf_firefly_image_host", "surf_debug_firefly_time"):
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("SvgfExt", "svgf_ext", "firefly_image_host", "svgf_image_host"):
        assert hasattr(surf_amd, name), name
    for name in ("firefly_image", "debug_firefly_time", "svgf", "svgf_image", "copy_svgf_to"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_ext():
    x = surf_amd.SvgfExt(7.0, 1)
    assert C.sizeof(x) == 16
    assert surf_amd.load().surf_svgf_default_ext(C.byref(x)) == 0
    assert bytes(x) == bytes(16)
    assert surf_amd.load().surf_svgf_default_ext(None) == SURF_ERR_INVALID
    y = surf_amd.svgf_ext(firefly_scale=4, feedback=True)
    assert (F(y.firefly_scale), y.feedback) == (F(4.0), 1)
    with pytest.raises(TypeError):
        surf_amd.svgf_image_host({}, None, ext=y, feedback=True)
    with pytest.raises(TypeError):
        surf_amd.svgf_image_host({}, None, ext=4.0)


def test_invalid_arguments_are_status_codes(svgf_frames, firefly_fixtures):
    lib = surf_amd.load()
    f0, f1 = svgf_frames["small"]
    ones = np.ones((3, 5, 4), np.float32)
    w, h, cur, prev, keep = surf_amd._svgf_frames(f1, with_moments(f0, ones, ones))
    o = [np.zeros((h, w, 4), np.float32) for _ in range(4)]
    op = [a.ctypes.data for a in o]
    tp, sp = surf_amd.temporal_params(), surf_amd.svgf_params()
    host = lib.surf_svgf_image_host_ex
    cb, pb, tb, gb = C.byref(cur), C.byref(prev), C.byref(tp), C.byref(sp)
    for scale, fb in ((0.0, 0), (-0.0, 0), (1.0, 1), (4.0, 0), (3.0e38, 1)):
        assert host(w, h, cb, pb, tb, gb, C.byref(surf_amd.svgf_ext(scale, fb)), *op) == 0, (scale, fb)
    assert host(w, h, cb, pb, tb, gb, None, *op) == 0
    for scale in (0.5, 0.99999, -1.0, -4.0, 1e-30, float("nan"), float("inf"), float("-inf")):
        assert host(w, h, cb, pb, tb, gb, C.byref(surf_amd.svgf_ext(scale, 0)), *op) == SURF_ERR_INVALID, scale
    for fb in (2, 0xFFFFFFFF):
        assert host(w, h, cb, pb, tb, gb, C.byref(surf_amd.svgf_ext(0.0, fb)), *op) == SURF_ERR_INVALID, fb
    good = C.byref(surf_amd.svgf_ext(4.0, 1))
    # the checks of the call without _ex hold
    assert host(w, h, None, pb, tb, gb, good, *op) == SURF_ERR_INVALID
    assert host(w, h, cb, pb, None, gb, good, *op) == SURF_ERR_INVALID
    assert host(w, h, cb, pb, tb, None, good, *op) == SURF_ERR_INVALID
    assert host(0, h, cb, pb, tb, gb, good, *op) == SURF_ERR_INVALID
    for k in range(4):
        args = list(op)
        args[k] = None
        assert host(w, h, cb, pb, tb, gb, good, *args) == SURF_ERR_INVALID, k
    assert host(w, h, cb, pb, tb, C.byref(surf_amd.svgf_params(spatial_below=0)), good, *op) == SURF_ERR_INVALID
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.svgf_image_host(f1, None, firefly_scale=0.5)
    assert e.value.code == SURF_ERR_INVALID and "firefly_scale" in str(e.value)
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.svgf_image_host(f1, None, ext=surf_amd.SvgfExt(0.0, 2))
    assert e.value.code == SURF_ERR_INVALID and "feedback" in str(e.value)
    # the clamp alone
    acc, alb = (np.ascontiguousarray(a) for a in firefly_fixtures["tile"])
    out = np.zeros_like(acc)
    fh = lib.surf_firefly_image_host
    ap, bp, outp = acc.ctypes.data, alb.ctypes.data, out.ctypes.data
    assert fh(33, 9, ap, bp, 1, 1.0, outp) == 0
    assert fh(33, 9, None, bp, 1, 1.0, outp) == SURF_ERR_INVALID
    assert fh(33, 9, ap, None, 1, 1.0, outp) == SURF_ERR_INVALID
    assert fh(33, 9, ap, bp, 1, 1.0, None) == SURF_ERR_INVALID
    assert fh(0, 9, ap, bp, 1, 1.0, outp) == SURF_ERR_INVALID
    assert fh(33, 0, ap, bp, 1, 1.0, outp) == SURF_ERR_INVALID
    for scale in (0.0, 0.5, -2.0, float("nan"), float("inf")):
        assert fh(33, 9, ap, bp, 1, scale, outp) == SURF_ERR_INVALID, scale
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.firefly_image_host(acc, alb, 0.0)
    assert e.value.code == SURF_ERR_INVALID and "scale" in str(e.value)
    # a NULL context
    assert lib.surf_svgf_accumulate_ex(None, tb, gb, good, op[0]) == SURF_ERR_INVALID
    assert lib.surf_svgf_copy_device_ex(None, tb, gb, good, op[0]) == SURF_ERR_INVALID
    assert lib.surf_svgf_image_ex(None, w, h, cb, pb, tb, gb, good, *op) == SURF_ERR_INVALID
    assert lib.surf_firefly_image(None, 33, 9, ap, bp, 1, 4.0, outp) == SURF_ERR_INVALID
    ms = C.c_float()
    assert lib.surf_debug_firefly_time(None, C.byref(ms)) == SURF_ERR_INVALID
    del keep


# ---- 2. the clamp's twin equals numpy, bit for bit ---------------------------------------

@pytest.mark.parametrize("scale", [1.0, 2.0, 4.0])
def test_clamp_on_a_real_frame(firefly_fixtures, scale):
    """The oracle's indoor frame 0, 100 x 37, 1 spp: 419 / 185 / 73 of its pixels exceed 1 / 2 / 4
    times their brightest neighbour (counted on the oracle's planes, independently of np_firefly)."""
    acc, alb = firefly_fixtures["real"]
    want, cnt = np_firefly(acc, alb, scale)
    print(scale, cnt)
    assert cnt["clamped"] == {1.0: 419, 2.0: 185, 4.0: 73}[scale] and cnt["unclamped"] > 3000
    got = surf_amd.firefly_image_host(acc, alb, scale)
    assert_images_equal(got, want, f"scale {scale}")
    changed = (got[..., :3] != acc[..., :3] / acc[..., 3:4]).any(-1)
    assert changed.sum() <= cnt["clamped"] and changed.sum() > 0.9 * cnt["clamped"]     # a clamped black pixel (l = lim = 0 fails l > lim) aside


@pytest.mark.parametrize("name,scale,demodulate", [("synthetic", 1.0, 1), ("synthetic", 4.0, 1), ("synthetic", 2.0, 0), ("one", 1.0, 1),
                                                   ("tile", 1.0, 1), ("tile", 1.5, 0), ("real", 2.0, 0)])
def test_clamp_synthetic_cases(firefly_fixtures, name, scale, demodulate):
    acc, alb = firefly_fixtures[name]
    want, cnt = np_firefly(acc, alb, scale, demodulate)
    got = surf_amd.firefly_image_host(acc, alb, scale, demodulate)
    assert_images_equal(got, want, f"{name}, scale {scale}, demodulate {demodulate}")
    if name == "one":
        assert cnt["cnt_zero"] == 1 and np.array_equal(got, acc)             # no neighbour: unchanged, (c, 1) = (A / 1, 1)


def test_clamp_fixtures_reach_every_branch(firefly_fixtures):
    acc, alb = firefly_fixtures["synthetic"]
    out, cnt = np_firefly(acc, alb, 4.0)
    print(cnt)
    assert cnt["invalid_centre"] == 66 and cnt["unsampled_centre"] == 10
    assert cnt["skipped_neighbours"] > 100 and cnt["cnt_zero"] == 1 and cnt["nan_stays"] == 1
    assert cnt["clamped"] > 30 and cnt["unclamped"] > 3000
    assert np.isnan(out[30, 40, :3]).all() and out[30, 40, 3] == 1.0                 # the NaN stays, its neighbours do not take it up
    assert not np.isnan(out[29:32, 39:42][np.arange(9).reshape(3, 3) != 4]).any()
    assert (out[0, 0] == 0.0).all() and (out[3, 70] == 0.0).all()                   # A.w == 0: (0, 0, 0, 0)
    assert np.array_equal(out[25, 50, :3], acc[25, 50, :3] / acc[25, 50, 3])        # cnt == 0: unchanged
    inv = out[10:16, 20:31]
    assert np.array_equal(inv[..., :3], acc[10:16, 20:31, :3] / acc[10:16, 20:31, 3:4])   # an invalid centre is never clamped
    t_out, t_cnt = np_firefly(*firefly_fixtures["tile"], 1.0)
    assert t_cnt["clamped"] > 20 and t_cnt["unclamped"] > 20                        # 33 x 9: both branches


# ---- 3. the chain: the _ex twin equals numpy, all four outputs ----------------------------

@pytest.mark.parametrize("ext", list(EXTS), ids=list(EXTS))
def test_chain_bitexact(svgf_frames, ext):
    want = expected_ext_chain(svgf_frames, "chain", 3, EXTS[ext], **CHAIN)
    prev = None
    for k, f in enumerate(svgf_frames["chain"][:3]):
        got = surf_amd.svgf_image_host(f, prev, **EXTS[ext], **CHAIN)
        assert_outputs_equal(got, want[k], f"ext {ext}, frame {k}")
        prev = with_moments(f, want[k][1], want[k][2])
    if "feedback" in EXTS[ext]:
        plain = expected_ext_chain(svgf_frames, "chain", 3, {k: v for k, v in EXTS[ext].items() if k != "feedback"}, **CHAIN)
        assert want[0][4]["fed_back"] > 3000
        assert_images_equal(want[0][0], plain[0][0], "feedback leaves the first frame's image alone")
        assert_images_equal(want[0][2], plain[0][2], "... and its moments")
        assert not np.array_equal(want[0][1], plain[0][1]) and not np.array_equal(want[1][0], plain[1][0])
        assert np.array_equal(want[1][1][..., 3], plain[1][1][..., 3])              # n' is unchanged


def test_one_iteration_feeds_back_the_output(svgf_frames):
    f0, f1 = svgf_frames["chain"][:2]
    params = dict(iterations=1, **CHAIN)
    first = surf_amd.svgf_image_host(f0, None, feedback=True, **params)
    assert_outputs_equal(first, np_svgf_ext(f0, None, feedback=True, **params), "frame 0")
    prev = with_moments(f0, first[1], first[2])
    got = surf_amd.svgf_image_host(f1, prev, feedback=True, **params)
    assert_outputs_equal(got, np_svgf_ext(f1, prev, feedback=True, **params), "frame 1")
    valid = f1["albedo"][..., 3] != 0
    assert valid.sum() > 3000
    assert np.array_equal(got[1][valid][:, :3].view(np.uint32), got[0][valid][:, :3].view(np.uint32))


# ---- 4. off means the call without _ex ------------------------------------------------------

@pytest.mark.parametrize("name,params", [("chain", CHAIN), ("tile", dict(iterations=6)), ("a", dict(demodulate=0))])
def test_off_is_the_plain_call(svgf_frames, name, params):
    prev = None
    for k, f in enumerate(svgf_frames[name][:3]):
        plain = surf_amd.svgf_image_host(f, prev, **params)
        for what, kw in (("all-zero ext", dict(ext=surf_amd.SvgfExt())), ("NULL ext", dict(ext=None)),
                         ("keywords off", dict(firefly_scale=0.0, feedback=False))):
            assert_outputs_equal(surf_amd.svgf_image_host(f, prev, **kw, **params), plain, f"{name}, frame {k}: {what}")
        prev = with_moments(f, plain[1], plain[2])


# ---- 5. quality -----------------------------------------------------------------------------

PLANTED = [(y, x) for y in (6, 16, 26) for x in (12, 37, 62, 87)]        # 12 pixels, 10 rows / 25 columns apart
# the twin's measured ratios x 1.15, rounded up to two decimals, as tests/test_svgf_host.py sets its own on the same frames
RATIO_FIRST_FRAME_CLAMP = 1.23        # measured 1.0695
RATIO_EIGHT_FRAMES_FEEDBACK = 1.20    # measured 1.0433
RATIO_EIGHT_FRAMES_BOTH = 1.30        # measured 1.1291


@pytest.fixture(scope="module")
def animation():
    """The 8 frames of tests/test_svgf_host.py's quality test -- the oracle's indoor scene at
    100 x 37, 1 spp per frame, update(0.05) before each -- with the 512-spp references of the
    first and the last pose and the emitter mask of the first."""
    osc = oracle.OracleScene()
    oracle.set_zero_cutoff(True)
    try:
        ubo = osc.camera_ubo(W, H)
        mats = osc.export()["materials"]
        table = np.frombuffer(mats, np.float32).reshape(-1, 16)
        frames, refs = [], {}
        for j in range(8):
            osc.update(0.05)
            f = frame_of(osc, ubo, W, H, oracle_colour(osc, W, H, j))
            f["albedo"] = albedo_of(f["id"], mats)
            frames.append(f)
            if j in (0, 7):
                osc.camera_ubo(W, H)
                ref_acc = osc.render(W, H, 1, first_frame=1000, spp=512, max_segments=64)[0]
                refs[j] = ref_acc[..., :3].astype(np.float64) / ref_acc[..., 3:4]
        ids = frames[0]["id"]
        emitter = (ids[..., 0] != 0xFFFFFFFF) & (table[np.where(ids[..., 0] != 0xFFFFFFFF, ids[..., 2], 0), 0] > 0)
    finally:
        oracle.set_zero_cutoff(False)
        osc.close()
    return frames, refs, emitter


def mae(img, ref):
    return float(np.abs(img[..., :3].astype(np.float64) - ref).mean())


def run_twin(frames, **ext):
    """The host twin along the frames, its own history and moments fed forward: the last frame's image."""
    prev = None
    for f in frames:
        out, hist, mom, _ = surf_amd.svgf_image_host(f, prev, **ext)
        prev = with_moments(f, hist, mom)
    return out


def test_planted_fireflies_are_clamped(animation):
    """12 samples of 1000 times their value, planted in the first frame's accumulator at valid,
    sampled, non-emitter pixels at least 3 apart: with firefly_scale 4 the filtered frame is
    closer to the 512-spp reference than the same input filtered without the clamp -- on the
    numpy restatement first, then on the twin.  Measured (deterministic): MAE 0.1239 with the clamp off, 0.0238 with firefly_scale 4;
    the unplanted frame without the clamp has 0.0235."""
    frames, refs, emitter = animation
    f0 = frames[0]
    acc = f0["acc"].copy()
    for a in PLANTED:
        assert f0["albedo"][a][3] != 0 and f0["acc"][a][3] > 0 and not emitter[a] and f0["acc"][a][:3].max() > 0, a
        for b in PLANTED:
            assert a == b or max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 3
        acc[a][:3] *= F(1000.0)
    planted = {**f0, "acc": acc}
    np_off, np_on = np_svgf_ext(planted, None)[0], np_svgf_ext(planted, None, firefly_scale=4.0)[0]
    e_off, e_on = mae(np_off, refs[0]), mae(np_on, refs[0])
    print(f"planted fireflies, first frame, MAE: clamp off {e_off:.4f}, firefly_scale 4 {e_on:.4f}; unplanted, clamp off "
          f"{mae(np_svgf(f0, None)[0], refs[0]):.4f}")
    assert e_on < e_off, (e_on, e_off)
    t_off, t_on = surf_amd.svgf_image_host(planted, None), surf_amd.svgf_image_host(planted, None, firefly_scale=4.0)
    assert_images_equal(t_off[0], np_off, "the twin, clamp off")
    assert_images_equal(t_on[0], np_on, "the twin, firefly_scale 4")
    assert mae(t_on[0], refs[0]) < mae(t_off[0], refs[0])


def test_clamp_on_the_first_real_frame(animation):
    """MAE against 512 spp of the first frame, firefly_scale 4 over the plain filter.
    Measured (deterministic): plain 0.0235, firefly_scale 4 0.0251, ratio 1.0695 -- ABOVE 1: on a
    frame without planted outliers the clamp costs more in removed energy (8 % of the frame's
    luminance at scale 4, test_energy_the_clamp_removes) than the 73 pixels it clamps gain.  The
    stage stays off by default.  Asserted <= 1.23 (the ratio x 1.15, rounded up)."""
    frames, refs, _ = animation
    plain, ext = mae(run_twin(frames[:1]), refs[0]), mae(run_twin(frames[:1], firefly_scale=4.0), refs[0])
    print(f"first frame: plain {plain:.4f}, firefly_scale 4 {ext:.4f}, ratio {ext / plain:.4f}")
    assert ext / plain <= RATIO_FIRST_FRAME_CLAMP, (ext, plain)


def test_feedback_after_eight_frames(animation):
    """MAE against 512 spp of the eighth frame, over the plain filter's, with feedback alone and
    with firefly_scale 4 as well.  Measured (deterministic): plain 0.0171, feedback 0.0178 (ratio
    1.0433), both 0.0193 (ratio 1.1291), the clamp alone 0.0182 (1.0667) -- every ratio ABOVE 1 at
    this size and sample count: the fed-back history is smoother but carries the first
    iteration's blur into every later frame.  Both stages stay off by default.  Asserted <= 1.20
    and <= 1.30 (the ratios x 1.15, rounded up)."""
    frames, refs, _ = animation
    plain = mae(run_twin(frames), refs[7])
    fb, both = mae(run_twin(frames, feedback=True), refs[7]), mae(run_twin(frames, firefly_scale=4.0, feedback=True), refs[7])
    clamp = mae(run_twin(frames, firefly_scale=4.0), refs[7])
    print(f"eighth frame: plain {plain:.4f}, feedback {fb:.4f} (ratio {fb / plain:.4f}), both {both:.4f} (ratio {both / plain:.4f}), "
          f"clamp alone {clamp:.4f} (ratio {clamp / plain:.4f})")
    assert fb / plain <= RATIO_EIGHT_FRAMES_FEEDBACK, (fb, plain)
    assert both / plain <= RATIO_EIGHT_FRAMES_BOTH, (both, plain)


def test_energy_the_clamp_removes(animation):
    """sum lum(A') / sum lum(A) over the 8 frames -- the clamp only ever lowers a pixel, and by
    less the larger the scale.  Measured: 0.8394 at scale 2, 0.9181 at scale 4."""
    frames, _, _ = animation
    kept = {}
    for scale in (2.0, 4.0):
        after = before = 0.0
        for f in frames:
            out = surf_amd.firefly_image_host(f["acc"], f["albedo"], scale)
            c = f["acc"][..., :3] / f["acc"][..., 3:4]
            assert (out[..., :3] <= c).all()
            after += float(lum(out[..., :3]).astype(np.float64).sum())
            before += float(lum(c).astype(np.float64).sum())
        kept[scale] = after / before
    print(f"energy kept over 8 frames: {kept}")
    assert kept[2.0] < kept[4.0] < 1.0
