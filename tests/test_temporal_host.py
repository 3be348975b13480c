"""Temporal accumulation with reprojection (surf_temporal*, include/surf_hip.h)
where it needs no GPU: exported symbols and defaults, status codes, the CPU twin
(surf_temporal_image_host) against a numpy restatement, the static-scene
behaviour and the filter's gain on an animated sequence of the oracle's indoor
scene.  CPU only.

Bar: bit-exact.  The expected images never come from the code under test:
np_temporal below restates the header's arithmetic, every step an explicit
float32 numpy operation (single IEEE operations, no contraction; np.rint
rounds to nearest even, np.floor is exact) in the stated order.  Images are
compared as uint32 words.

tests/test_gpu_temporal.py imports np_temporal and the frames from here.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import surf_amd
from test_denoise_host import assert_images_equal
from test_gpu_aov import expected_planes

F = np.float32
UNSET = 0xFFFFFFFF
SURF_ERR_INVALID = -1
W, H = 100, 37
DEFAULTS = dict(alpha_min=0.0, max_history=32, normal_min=0.9, plane_tol=0.01, snap=1.0 / 64.0, min_weight=0.01)
CHAIN = dict(max_history=3, alpha_min=0.4)          # both clamps bind within six frames
FAR_STEP = (0.5, 0.2, 0.0)                          # a camera step sideways that takes the frame's edge pixels outside the previous frame
ZERO_PIXEL = (H // 2, W // 3)                       # its accumulator is emptied in some frames (A.w == 0)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def np_temporal(cur, prev, alpha_min=0.0, max_history=32, normal_min=0.9, plane_tol=0.01, snap=1.0 / 64.0, min_weight=0.01):
    """The header's arithmetic.  cur: dict of 'acc', 'position', 'normal' ((H, W, 4)
    float32), 'id' ((H, W, 4) uint32), 'instances' (bytes); prev: None or a dict of
    'history', 'position', 'normal', 'id', 'instances', 'camera' (128 bytes).
    Returns (out, hist, counts): counts says how many pixels took each branch."""
    A, P, N = (np.asarray(cur[k], np.float32) for k in ("acc", "position", "normal"))
    ID = np.asarray(cur["id"], np.uint32)[..., 0]
    h, w = ID.shape
    alpha_min, normal_min, plane_tol, snap, min_weight = (F(v) for v in (alpha_min, normal_min, plane_tol, snap, min_weight))
    maxh = F(max_history)
    cnt = {}
    with np.errstate(all="ignore"):
        # 1. colour
        inv = np.where(A[..., 3] > F(0.0), F(1.0) / A[..., 3], F(0.0)).astype(np.float32)
        c = A[..., :3] * inv[..., None]
        # 2. misses
        miss = ID == UNSET
        sum_w, sum_n, sum_c = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 3), np.float32)
        cnt["miss"] = int(miss.sum())
        if prev is not None:
            ci = np.frombuffer(cur["instances"], np.float32).reshape(-1, 40)
            pi = np.frombuffer(prev["instances"], np.float32).reshape(-1, 40)
            assert ci.shape == pi.shape
            n_inst = len(ci)
            Pprev, Nprev = P[..., :3], N[..., :3]
            moved = np.zeros((h, w), bool)
            if n_inst:
                moved_i = (ci.view(np.uint32)[:, 8:40] != pi.view(np.uint32)[:, 8:40]).any(axis=1)    # transform @32, inv_transform @96
                idc = np.where(ID < n_inst, ID, 0)
                moved = ~miss & (ID < n_inst) & moved_i[idc]
                # 3. previous position and normal of moved pixels
                V, T = ci[idc, 24:40], pi[idc, 8:24]
                Px, Py, Pz = P[..., 0], P[..., 1], P[..., 2]
                q = [((V[..., k] * Px + V[..., 4 + k] * Py) + V[..., 8 + k] * Pz) + V[..., 12 + k] for k in range(3)]
                pm = [((T[..., k] * q[0] + T[..., 4 + k] * q[1]) + T[..., 8 + k] * q[2]) + T[..., 12 + k] for k in range(3)]
                Nx, Ny, Nz = N[..., 0], N[..., 1], N[..., 2]
                qn = [(V[..., k] * Nx + V[..., 4 + k] * Ny) + V[..., 8 + k] * Nz for k in range(3)]
                m = [(T[..., k] * qn[0] + T[..., 4 + k] * qn[1]) + T[..., 8 + k] * qn[2] for k in range(3)]
                il = F(1.0) / np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
                nm = [m[k] * il for k in range(3)]
                Pprev = np.where(moved[..., None], np.stack(pm, axis=-1), Pprev)
                Nprev = np.where(moved[..., None], np.stack(nm, axis=-1), Nprev)
            cnt["moved"] = int(moved.sum())
            assert Pprev.dtype == np.float32 and Nprev.dtype == np.float32
            # host constants of the previous camera
            cam = np.frombuffer(prev["camera"], np.float32)
            Cc, F0, U, Vv, res = cam[0:3], cam[16:19], cam[20:23], cam[24:27], cam[28:30]
            G = F0 - Cc
            nrm = np.array([U[1] * Vv[2] - U[2] * Vv[1], U[2] * Vv[0] - U[0] * Vv[2], U[0] * Vv[1] - U[1] * Vv[0]], np.float32)
            g = (G[0] * nrm[0] + G[1] * nrm[1]) + G[2] * nrm[2]
            iu = F(1.0) / ((U[0] * U[0] + U[1] * U[1]) + U[2] * U[2])
            iv = F(1.0) / ((Vv[0] * Vv[0] + Vv[1] * Vv[1]) + Vv[2] * Vv[2])
            assert all(type(k) is np.float32 for k in (g, iu, iv))
            # 4. projection
            D = Pprev - Cc
            dn = dot3(D, nrm)
            s = g / dn
            Hh = D * s[..., None] - G
            fx = (dot3(Hh, U) * iu) * res[0]
            fy = (dot3(Hh, Vv) * iv) * res[1]
            ok = ~miss & (s > F(0.0)) & (fx > F(-1.0)) & (fx < F(w)) & (fy > F(-1.0)) & (fy < F(h))
            cnt["outside"] = int((~miss & ~ok).sum())
            fx, fy = np.where(ok, fx, F(0.0)), np.where(ok, fy, F(0.0))
            # 5. snap
            rx, ry = np.rint(fx), np.rint(fy)
            snx, sny = np.abs(fx - rx) <= snap, np.abs(fy - ry) <= snap
            fx, fy = np.where(snx, rx, fx), np.where(sny, ry, fy)
            cnt["snapped"] = int((ok & (snx | sny)).sum())
            cnt["snapped_both"] = int((ok & snx & sny).sum())
            # 6. taps
            flx, fly = np.floor(fx), np.floor(fy)
            ix, iy = flx.astype(np.int64), fly.astype(np.int64)
            tx, ty = fx - flx, fy - fly
            wx, wy = [F(1.0) - tx, tx], [F(1.0) - ty, ty]
            tol = plane_tol * P[..., 3]
            pH, pP, pN = (np.asarray(prev[k], np.float32) for k in ("history", "position", "normal"))
            pID = np.asarray(prev["id"], np.uint32)[..., 0]
            cand, used = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
            for t in range(4):
                qx, qy = ix + (t & 1), iy + (t >> 1)
                wgt = wx[t & 1] * wy[t >> 1]
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (wgt > F(0.0))
                xc, yc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                Hq, Pq, Nq, Iq = pH[yc, xc], pP[yc, xc][..., :3], pN[yc, xc][..., :3], pID[yc, xc]
                dnn = dot3(Nq, Nprev)
                pl = dot3(Pprev - Pq, Nq)
                use = inside & (Iq == ID) & (Hq[..., 3] > F(0.0)) & (dnn >= normal_min) & (np.abs(pl) <= tol)
                sum_w = np.where(use, sum_w + wgt, sum_w)
                sum_c = np.where(use[..., None], sum_c + wgt[..., None] * Hq[..., :3], sum_c)
                sum_n = np.where(use, sum_n + wgt * Hq[..., 3], sum_n)
                cand += inside
                used += use
            cnt["partial_taps"] = int(((cand == 4) & (used >= 1) & (used <= 3)).sum())
        # 7. blend
        have = ~miss & (sum_w > min_weight)
        hc = sum_c / sum_w[..., None]
        hn = sum_n / sum_w
        sampled = A[..., 3] > F(0.0)
        nn = hn + F(1.0)
        n1 = np.where(nn < maxh, nn, maxh)
        a0 = F(1.0) / n1
        a = np.where(a0 < alpha_min, alpha_min, a0)
        blend = hc + (c - hc) * a[..., None]
        r = np.where((have & sampled)[..., None], blend, np.where((have & ~sampled)[..., None], hc, c))
        nout = np.where(have & sampled, n1, np.where(have & ~sampled, hn, np.where(sampled, F(1.0), F(0.0))))
        nout = np.where(miss, F(0.0), nout)
        cnt["disoccluded"] = int((~miss & ~have).sum()) if prev is not None else 0
        cnt["empty_with_history"] = int((have & ~sampled).sum())
        cnt["empty_without_history"] = int((~miss & ~have & ~sampled).sum())
        cnt["history_clamped"] = int((have & sampled & (nn > maxh)).sum())
        cnt["alpha_clamped"] = int((have & sampled & (a0 < alpha_min)).sum())
    for arr in (r, nout, c):
        assert arr.dtype == np.float32
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = r
    hist = out.copy()
    hist[..., 3] = nout
    return out, hist, cnt


# ---- the frames ---------------------------------------------------------------

def shifted(ubo: bytes, shift) -> bytes:
    """The camera moved by `shift` (position and first_pixel)."""
    u = np.frombuffer(ubo, np.float32).copy()
    s = np.asarray(shift, np.float32)
    u[0:3] = u[0:3] + s
    u[16:19] = u[16:19] + s
    return u.tobytes()


def frame_of(osc, ubo, w, h, acc):
    """A frame as np_temporal and the bindings take it, from the oracle's planes of its current pose."""
    planes, _ = expected_planes(osc, ubo, w, range(h))
    f = {"acc": np.ascontiguousarray(acc, np.float32), "position": planes["position"], "normal": planes["normal"], "id": planes["id"],
         "instances": osc.export()["instances"], "camera": ubo}
    for a in f.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return f


def as_prev(frame, history):
    return {"history": history, "position": frame["position"], "normal": frame["normal"], "id": frame["id"],
            "instances": frame["instances"], "camera": frame["camera"]}


def oracle_colour(osc, w, h, k, spp=1):
    osc.camera_ubo(w, h)
    return osc.render(w, h, 1, first_frame=k * spp, spp=spp, max_segments=64)[0]


def emptied(acc, pixel=ZERO_PIXEL):
    a = acc.copy()
    a[pixel] = 0.0
    return a


@pytest.fixture(scope="session")
def temporal_frames():
    """name -> list of frames (shared, read only), each pair (k, k+1) a case:
    'a' two poses update(0.1) apart; 'b' the same with the camera also shifted;
    'c' a far camera under which 30 - 80 % of the pixels miss, seeded colour;
    'small' / 'tile' 5 x 3 and 33 x 9; 'chain' six frames, the instance moving
    every frame and the camera in two of them."""
    osc = oracle.OracleScene()
    oracle.set_zero_cutoff(True)
    try:
        ubo = osc.camera_ubo(W, H)
        small = {"small": (5, 3), "tile": (33, 9)}
        ubos = {k: osc.camera_ubo(*v) for k, v in small.items()}
        rng = np.random.default_rng(7)
        far = shifted(ubo, (0.0, 6.0, -12.0))

        def random_acc(w, h):
            a = np.empty((h, w, 4), np.float32)
            a[..., :3] = rng.uniform(0.0, 8.0, (h, w, 3)).astype(np.float32)
            a[..., 3] = F(2.0)
            return a

        frames = {k: [] for k in ("a", "b", "c", "small", "tile", "chain")}
        # pose 0
        c0 = oracle_colour(osc, W, H, 0)
        frames["a"].append(frame_of(osc, ubo, W, H, c0))
        frames["b"].append(frames["a"][0])
        frames["c"].append(frame_of(osc, far, W, H, random_acc(W, H)))
        for k, (w, h) in small.items():
            frames[k].append(frame_of(osc, ubos[k], w, h, random_acc(w, h)))
        frames["chain"].append(frame_of(osc, ubo, W, H, emptied(c0)))
        # pose 1 .. 5
        cam = ubo
        for j in range(1, 6):
            osc.update(0.1)
            cj = oracle_colour(osc, W, H, j)
            if j == 1:
                frames["a"].append(frame_of(osc, ubo, W, H, emptied(cj)))
                frames["b"].append(frame_of(osc, shifted(ubo, (0.05, 0.02, 0.03)), W, H, cj))
                frames["c"].append(frame_of(osc, shifted(far, FAR_STEP), W, H, random_acc(W, H)))
                for k, (w, h) in small.items():
                    frames[k].append(frame_of(osc, shifted(ubos[k], (0.05, 0.02, 0.03)), w, h, random_acc(w, h)))
            if j in (2, 4):
                cam = shifted(cam, (0.05, 0.02, 0.03) if j == 2 else FAR_STEP)
            frames["chain"].append(frame_of(osc, cam, W, H, emptied(cj) if j in (1, 3) else cj))
    finally:
        oracle.set_zero_cutoff(False)
        osc.close()
    return frames


_chains = {}


def expected_chain(frames, name, **params):
    """[(out, hist, counts)] of np_temporal along a list of frames, the numpy history fed forward; computed once."""
    key = (name, tuple(sorted(params.items())))
    if key not in _chains:
        res, prev = [], None
        for f in frames[name]:
            out, hist, cnt = np_temporal(f, prev, **{**DEFAULTS, **params})
            out.setflags(write=False)
            hist.setflags(write=False)
            res.append((out, hist, cnt))
            prev = as_prev(f, hist)
        _chains[key] = res
    return _chains[key]


CASES = [("a", {}), ("b", {}), ("c", {}), ("small", {}), ("tile", {}), ("chain", CHAIN)]


# ---- 1. symbols and defaults ---------------------------------------------------

def test_symbols_exported_at_abi_4():
    lib = surf_amd.load()
    for name in ("surf_temporal_default_params", "surf_temporal_accumulate", "surf_temporal_copy_device", "surf_temporal_reset",
                 "surf_temporal_history", "surf_temporal_image", "surf_temporal_image_host", "surf_debug_temporal_time"):
        assert hasattr(lib, name), name
    assert lib.surf_abi_version() == 4
    for name in ("TemporalParams", "temporal_params", "temporal_image_host"):
        assert hasattr(surf_amd, name), name
    for name in ("temporal", "temporal_reset", "temporal_history", "temporal_image", "copy_temporal_to", "debug_temporal_time"):
        assert hasattr(surf_amd.Renderer, name), name


def test_default_params():
    p = surf_amd.TemporalParams()
    assert C.sizeof(p) == 32
    assert surf_amd.load().surf_temporal_default_params(C.byref(p)) == 0
    assert p.max_history == 32
    assert (F(p.alpha_min), F(p.normal_min), F(p.plane_tol), F(p.snap), F(p.min_weight)) == (F(0.0), F(0.9), F(0.01), F(1.0 / 64.0), F(0.01))
    q = surf_amd.temporal_params(max_history=3, alpha_min=0.25)
    assert (q.max_history, F(q.alpha_min), F(q.normal_min)) == (3, F(0.25), F(0.9))
    with pytest.raises(TypeError):
        surf_amd.temporal_params(sigma=1.0)


# ---- 2. error paths --------------------------------------------------------------

def test_invalid_arguments_are_status_codes(temporal_frames):
    lib = surf_amd.load()
    f0, f1 = temporal_frames["small"]
    w, h, cur, prev, keep = surf_amd._temporal_frames(f1, as_prev(f0, np.ones((3, 5, 4), np.float32)))
    out, hist = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    good = surf_amd.temporal_params()
    host = lib.surf_temporal_image_host
    cb, pb, gb = C.byref(cur), C.byref(prev), C.byref(good)
    assert host(w, h, cb, pb, gb, out.ctypes.data, hist.ctypes.data) == 0
    assert host(w, h, cb, None, gb, out.ctypes.data, hist.ctypes.data) == 0            # a first frame
    assert host(w, h, None, pb, gb, out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID
    assert host(w, h, cb, pb, None, out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID
    assert host(w, h, cb, pb, gb, None, hist.ctypes.data) == SURF_ERR_INVALID
    assert host(w, h, cb, pb, gb, out.ctypes.data, None) == SURF_ERR_INVALID
    assert host(0, h, cb, pb, gb, out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID
    assert host(w, 0, cb, pb, gb, out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID
    for struct, fields in ((cur, ("acc", "position", "normal", "id", "instances")), (prev, ("history", "position", "normal", "id", "instances"))):
        for name in fields:                                                             # each plane NULL
            saved = getattr(struct, name)
            setattr(struct, name, None)
            assert host(w, h, cb, pb, gb, out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID, name
            setattr(struct, name, saved)
    prev.instance_count -= 1                                                            # counts differ between the frames
    assert host(w, h, cb, pb, gb, out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID
    assert b"instance counts" in lib.surf_last_error(None)
    prev.instance_count += 1
    bad = {"alpha_min": (-0.1, 1.5, float("nan")), "max_history": (0,), "normal_min": (-1.5, 1.5, float("nan")),
           "plane_tol": (0.0, -1.0, float("nan"), float("inf")), "min_weight": (0.0, -1.0, float("nan"), float("inf")),
           "snap": (-0.1, 0.5, 0.75, float("nan"))}
    for field, values in bad.items():
        for v in values:
            p = surf_amd.temporal_params(**{field: v})
            assert host(w, h, cb, pb, C.byref(p), out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID, (field, v)
    okay = {"alpha_min": (0.0, 1.0), "max_history": (1, 0xFFFFFFFF), "normal_min": (-1.0, 1.0), "snap": (0.0, 0.49)}
    for field, values in okay.items():
        for v in values:
            p = surf_amd.temporal_params(**{field: v})
            assert host(w, h, cb, pb, C.byref(p), out.ctypes.data, hist.ctypes.data) == 0, (field, v)
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.temporal_image_host(f1, None, max_history=0)
    assert e.value.code == SURF_ERR_INVALID and "max_history" in str(e.value)
    # a NULL context
    assert lib.surf_temporal_default_params(None) == SURF_ERR_INVALID
    assert lib.surf_temporal_accumulate(None, gb, None, out.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_temporal_copy_device(None, gb, None, out.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_temporal_reset(None) == SURF_ERR_INVALID
    assert lib.surf_temporal_history(None, out.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_temporal_image(None, w, h, cb, pb, gb, out.ctypes.data, hist.ctypes.data) == SURF_ERR_INVALID
    ms = C.c_float()
    assert lib.surf_debug_temporal_time(None, C.byref(ms)) == SURF_ERR_INVALID
    del keep


# ---- 3. the host twin equals numpy, bit for bit ----------------------------------

@pytest.mark.parametrize("name,params", CASES, ids=[c[0] for c in CASES])
def test_host_twin_bitexact(temporal_frames, name, params):
    want = expected_chain(temporal_frames, name, **params)
    prev = None
    for k, f in enumerate(temporal_frames[name]):
        out, hist = surf_amd.temporal_image_host(f, prev, **params)
        assert_images_equal(out, want[k][0], f"case {name}, frame {k}: out")
        assert_images_equal(hist, want[k][1], f"case {name}, frame {k}: history")
        assert (out[..., 3] == 1.0).all() and np.array_equal(out[..., :3], hist[..., :3])
        prev = as_prev(f, want[k][1])                         # the numpy history fed forward


def test_inputs_reach_every_branch(temporal_frames):
    a = expected_chain(temporal_frames, "a")[1][2]
    b = expected_chain(temporal_frames, "b")[1][2]
    c = expected_chain(temporal_frames, "c")[1][2]
    chain = [r[2] for r in expected_chain(temporal_frames, "chain", **CHAIN)]
    print({"a": a, "b": b, "c": c, "chain": chain})
    assert a["moved"] >= 20 and b["moved"] >= 20                 # the rotating Suzanne's pixels
    assert a["disoccluded"] > 0 and all(k["disoccluded"] > 0 for k in chain[1:])
    assert a["snapped_both"] > 1000 and b["snapped"] < a["snapped"]   # an unmoved camera snaps the unmoved pixels; a moved one few
    assert a["partial_taps"] > 0 and b["partial_taps"] > 0
    assert chain[4]["outside"] > 0                               # the camera's large step
    assert 0.3 * W * H <= c["miss"] <= 0.8 * W * H
    assert a["empty_with_history"] == 1                          # ZERO_PIXEL, whose first frame was sampled
    assert chain[0]["empty_without_history"] == 1 and chain[1]["empty_without_history"] == 1 and chain[3]["empty_with_history"] == 1
    assert sum(k["history_clamped"] for k in chain) > 0 and sum(k["alpha_clamped"] for k in chain) > 0


def test_first_frame_starts_every_history(temporal_frames):
    f = temporal_frames["a"][0]
    out, hist = surf_amd.temporal_image_host(f, None)
    hit = f["id"][..., 0] != UNSET
    c = f["acc"][..., :3] * (F(1.0) / f["acc"][..., 3:4])
    assert np.array_equal(out[..., :3], c)
    assert (hist[..., 3][hit] == 1.0).all() and (hist[..., 3][~hit] == 0.0).all()


# ---- 4. a static scene converges to the mean ----------------------------------------

def test_static_scene_accumulates_the_mean():
    """k = 6 frames, nothing moves, alpha_min 0, max_history 32: every hit pixel's
    history length is exactly k and its colour is the mean of the k frames within
    8 k 2^-24 max|c| (three roundings per blend plus that of 1/n', on magnitudes
    <= 2 max|c|, undamped; the snap makes each tap exact)."""
    k = 6
    osc = oracle.OracleScene()
    oracle.set_zero_cutoff(True)
    try:
        ubo = osc.camera_ubo(W, H)
        frames = [frame_of(osc, ubo, W, H, oracle_colour(osc, W, H, j)) for j in range(k)]
    finally:
        oracle.set_zero_cutoff(False)
        osc.close()
    prev = None
    for f in frames:
        out, hist = surf_amd.temporal_image_host(f, prev)
        prev = as_prev(f, hist)
    hit = frames[0]["id"][..., 0] != UNSET
    assert hit.sum() > 0.5 * W * H
    assert (hist[..., 3][hit] == F(k)).all(), np.unique(hist[..., 3][hit])
    cols = np.stack([f["acc"][..., :3].astype(np.float64) / f["acc"][..., 3:4] for f in frames])
    mean = cols.mean(axis=0)
    bound = 8 * k * 2.0 ** -24 * np.abs(cols).max()
    dev = np.abs(out[..., :3].astype(np.float64) - mean)[hit].max()
    print(f"static scene: max deviation from the mean {dev:.3e}, bound {bound:.3e}")
    assert dev <= bound, (dev, bound)
    assert np.array_equal(out[~hit][:, :3], (frames[-1]["acc"][..., :3] * (F(1.0) / frames[-1]["acc"][..., 3:4]))[~hit])


# ---- 5. quality ----------------------------------------------------------------------

def test_temporal_is_closer_to_the_converged_image():
    """mean |temporal - ref| <= 0.65 * mean |1 spp - ref| after 8 frames of
    update(0.05) at 1 spp per frame, 100 x 37, default parameters, against the
    oracle's 512-spp render of the last pose (np_temporal measures 0.530: 0.0481
    against 0.0907; the result is deterministic)."""
    osc = oracle.OracleScene()
    oracle.set_zero_cutoff(True)
    try:
        ubo = osc.camera_ubo(W, H)
        prev = None
        for j in range(8):
            osc.update(0.05)
            f = frame_of(osc, ubo, W, H, oracle_colour(osc, W, H, j))
            last_prev = prev
            out, hist, _ = np_temporal(f, prev)
            prev = as_prev(f, hist)
        assert_images_equal(surf_amd.temporal_image_host(f, last_prev)[0], out, "the host twin on the last frame")
        osc.camera_ubo(W, H)
        ref_acc = osc.render(W, H, 1, first_frame=1000, spp=512, max_segments=64)[0]
    finally:
        oracle.set_zero_cutoff(False)
        osc.close()
    noisy = f["acc"][..., :3] / f["acc"][..., 3:4]
    ref = ref_acc[..., :3].astype(np.float64) / ref_acc[..., 3:4]
    err_noisy = float(np.abs(noisy.astype(np.float64) - ref).mean())
    err_got = float(np.abs(out[..., :3].astype(np.float64) - ref).mean())
    print(f"mean abs error: 1 spp {err_noisy:.4f}, temporal {err_got:.4f}, ratio {err_got / err_noisy:.3f}")
    assert err_got <= 0.65 * err_noisy, (err_got, err_noisy)


# ---- 6. the example ------------------------------------------------------------------

def test_render_animated_example_is_built():
    exe = os.path.join(os.path.dirname(surf_amd.LIB_PATH), "..", "build", "render_animated")
    assert os.path.isfile(exe) and os.access(exe, os.X_OK)
