"""Sampled feature buffers (surf_read_aov_sampled / Renderer.aov_sampled())
against the CPU oracle plus numpy.

Bar: bit-exact, planes compared as uint32 words.  The expected planes never
come from the code under test:
  * the camera rays are restated here in numpy from the 128-byte camera UBO --
    initSeed, xorshift32, rndRange = (rndF * (hi - lo)) + lo, the lens disk's
    rejection loop, the view-plane point, normalise -- every step an explicit
    float32 operation, and PINNED to the oracle: for pixels spread over the
    image they equal, word for word, the first extension ray
    oracle_scene.record_rays records for that pixel and frame;
  * the oracle traces them (trace_closest) and the per-sample features are
    tests/test_gpu_aov.py's expected_planes arithmetic, restated for given rays;
  * the sums run in sample order in float32, the matte table as the header
    states it.

Frames are 100 x 37 (3,700 pixels: a partial last block of 256 lanes) unless
said otherwise.
"""
import ctypes as C
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

import oracle
import surf_amd

pytestmark = pytest.mark.gpu
UNSET = 0xFFFFFFFF
F = np.float32
U = np.uint32
W, H = 100, 37
PLANES = surf_amd.AOVS_PLANES
SLOTS, RANKS = 8, 4

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanf.argtypes, _libm.tanf.restype = [C.c_float], C.c_float


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


# ---- the camera sampler, restated (numpy uint32 / float32) -------------------

def wang_hash(s):
    s = (s ^ U(61)) ^ (s >> U(16))
    s = s * U(9)
    s = s ^ (s >> U(4))
    s = s * U(0x27d4eb2d)
    return s ^ (s >> U(15))


def init_seed(s):
    return wang_hash((s + U(1)) * U(0x11))


def rnd_u(s):
    s = s ^ (s << U(13))
    s = s ^ (s >> U(17))
    return s ^ (s << U(5))


def rnd_range(s, lo, hi):
    """(value, next state): (rndF(s) * (hi - lo)) + lo, rndF = (float)rndU * 2^-32."""
    s = rnd_u(s)
    r = F(hi) - F(lo)
    return (s.astype(np.float32) * F(2.3283064365387e-10)) * r + F(lo), s


def pixel_index(width, rows):
    rows = np.asarray(list(rows), np.uint32)
    x = np.tile(np.arange(width, dtype=np.uint32), len(rows))
    row = np.repeat(rows, width)
    return x, row


def sample_rays(ubo: bytes, width: int, rows, frame: int):
    """The render's primary ray of every pixel of `rows` in frame `frame` (one
    sample per frame): seed initSeed(p + 1799 * frame), jy, jx, the lens disk
    when the camera has a defocus angle."""
    c = np.frombuffer(ubo, np.float32)
    pos, up, fwd, first, uvec, vvec, res = c[0:3], c[4:7], c[8:11], c[16:19], c[20:23], c[24:27], c[28:30]
    focal, defocus = c[30], c[31]
    inv_w, inv_h = F(1.0) / res[0], F(1.0) / res[1]
    x, row = pixel_index(width, rows)
    with np.errstate(over="ignore"):
        p = x + row * U(width)
        seed = init_seed(p + U(1799) * U(frame & 0xFFFFFFFF))
        jy, seed = rnd_range(seed, -0.5, 0.5)
        jx, seed = rnd_range(seed, -0.5, 0.5)
        u, v = (x.astype(np.float32) + jx) * inv_w, (row.astype(np.float32) + jy) * inv_h
        n = len(x)
        o = np.broadcast_to(pos, (n, 3)).copy()
        if defocus != F(0.0):
            # sampleDefocusDisk's constants: right = normalize(cross(up, fwd)), radius = focal * tanf(radians(defocus / 2))
            cr = np.array([up[1] * fwd[2] - up[2] * fwd[1], up[2] * fwd[0] - up[0] * fwd[2], up[0] * fwd[1] - up[1] * fwd[0]], np.float32)
            inv = F(1.0) / np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
            right = cr * inv
            deg = defocus / F(2.0)
            radius = focal * F(_libm.tanf(float((deg * F(3.14159265358979323846264)) * F(0.005555555555555))))
            du, dv = right * radius, (F(-1.0) * up) * radius
            sx, sy = np.zeros(n, np.float32), np.zeros(n, np.float32)
            todo = np.ones(n, bool)
            while todo.any():
                ny, s1 = rnd_range(seed, -1.0, 1.0)
                nx, s2 = rnd_range(s1, -1.0, 1.0)
                sy, sx, seed = np.where(todo, ny, sy), np.where(todo, nx, sx), np.where(todo, s2, seed)
                todo = todo & (sx * sx + sy * sy > F(1.0))
            o = o + (sx[:, None] * du + sy[:, None] * dv)
        plane = (first + u[:, None] * uvec) + v[:, None] * vvec
        dirs = plane - o
        inv = F(1.0) / np.sqrt((dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2])
        d = dirs * inv[:, None]
    assert o.dtype == np.float32 and d.dtype == np.float32 and seed.dtype == np.uint32
    return o, d


def centre_rays(ubo: bytes, width: int, rows):
    """The unjittered ray of every pixel (the first-hit planes' ray), for the oracle-side checks."""
    c = np.frombuffer(ubo, np.float32)
    pos, first, uvec, vvec, res = c[0:3], c[16:19], c[20:23], c[24:27], c[28:30]
    x, row = pixel_index(width, rows)
    u, v = x.astype(np.float32) * (F(1.0) / res[0]), row.astype(np.float32) * (F(1.0) / res[1])
    dirs = ((first + u[:, None] * uvec) + v[:, None] * vvec) - pos
    d = dirs * (F(1.0) / np.sqrt((dirs * dirs).sum(axis=1, dtype=np.float32)))[:, None]
    return np.broadcast_to(pos, d.shape).copy(), d


def assert_rays_pinned(osc, ubo, width, height, frame, pixels):
    """The restated rays of `pixels` equal the oracle's recorded primary rays word for word."""
    o, d = sample_rays(ubo, width, range(height), frame)
    for p in pixels:
        (eo, ed), _ = osc.record_rays(width, height, frame, int(p), int(p) + 1, max_ext=4096, max_shadow=4096)
        assert len(eo) >= 1
        assert np.array_equal(eo[0].view(np.uint32), o[p].view(np.uint32)), (frame, p, eo[0], o[p])
        assert np.array_equal(ed[0].view(np.uint32), d[p].view(np.uint32)), (frame, p, ed[0], d[p])


SPREAD = np.unique(np.linspace(0, W * H - 1, 67).astype(np.int64))     # 67 pixels from corner to corner


# ---- the per-sample features (test_gpu_aov.py's expected_planes, for given rays) ----

def ray_features(osc, o, d):
    t, u, v, inst, prim = osc.trace_closest(o, d)
    ex = osc.export()
    inst_u = np.frombuffer(ex["instances"], np.uint32).reshape(-1, 40)    # tri_offset @0, material_offset @12
    inst_f = np.frombuffer(ex["instances"], np.float32).reshape(-1, 40)   # M column-major @32
    text = np.frombuffer(ex["tri_ext"], np.float32).reshape(-1, 20)       # n0 @0, n1 @16, n2 @32
    mats = np.frombuffer(ex["materials"], np.float32).reshape(-1, 16)     # strength @0, emission @16, albedo @32
    bg_u = np.frombuffer(ex["background"], np.uint32)
    bg_f = np.frombuffer(ex["background"], np.float32)                    # color @16, gradient A @32, B @48
    n = len(t)
    hit = inst != UNSET
    ii, pp = np.where(hit, inst, 0), np.where(hit, prim, 0)
    tri = inst_u[ii, 0] + pp
    mat = inst_u[ii, 3]
    col = lambda a: a[:, None]
    with np.errstate(all="ignore"):                                       # miss lanes compute discarded values
        P = o + col(t) * d
        n0, n1, n2 = text[tri, 0:3], text[tri, 4:7], text[tri, 8:11]
        w = (F(1.0) - u) - v
        no = (col(u) * n0 + col(v) * n2) + col(w) * n1
        M = inst_f[ii, 8:24]
        mrow = lambda i: (M[:, i] * no[:, 0] + M[:, 4 + i] * no[:, 1]) + (M[:, 8 + i] * no[:, 2] + M[:, 12 + i] * F(0.0))
        nx, ny, nz, nw = mrow(0), mrow(1), mrow(2), mrow(3)
        nn = (nx * nx + ny * ny) + (nz * nz + nw * nw)
        ninv = F(1.0) / np.sqrt(nn)
        N = np.stack([nx * ninv, ny * ninv, nz * ninv], axis=1)
        flip = ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]) > F(0.0)
        N = np.where(col(flip), N * F(-1.0), N)
        strength, ecol = mats[mat, 0], mats[mat, 4:7]
        emitter = (strength > F(0.0)) & ((ecol[:, 0] > F(0.0)) | (ecol[:, 1] > F(0.0)) | (ecol[:, 2] > F(0.0)))
        A = np.where(col(emitter), col(strength) * ecol, mats[mat, 8:11])
        bg = np.zeros((n, 3), np.float32)
        if bg_u[0] == 0:
            bg[:] = bg_f[4:7]
        elif bg_u[0] == 1:
            a = F(0.5) * (F(1.0) + d[:, 1])
            bg = col(a) * bg_f[12:15] + col(F(1.0) - a) * bg_f[8:11]
    a = np.where(col(hit), A, bg)
    for arr in (P, N, a, t):
        assert arr.dtype == np.float32
    return {"hit": hit, "P": P, "t": t, "N": N, "a": a, "inst": np.where(hit, inst, U(UNSET)).astype(np.uint32),
            "prim": np.where(hit, prim, U(UNSET)).astype(np.uint32), "mat": np.where(hit, mat, U(UNSET)).astype(np.uint32)}


class Expected:
    """Per-frame features of one (oracle scene, camera, rows), traced once per frame and shared."""

    def __init__(self, osc, ubo, width, rows):
        self.osc, self.ubo, self.width, self.rows = osc, ubo, width, list(rows)
        self.frames = {}

    def frame(self, f):
        if f not in self.frames:
            self.frames[f] = ray_features(self.osc, *sample_rays(self.ubo, self.width, self.rows, f))
        return self.frames[f]

    def planes(self, samples, first_sample=0, key="instance"):
        """(planes, info): the six planes as (rows, width, 4), and what the frame exercises."""
        fs = [self.frame((first_sample + s) & 0xFFFFFFFF) for s in range(samples)]
        n = len(fs[0]["hit"])
        col = lambda a: a[:, None]
        n_hit = np.zeros(n, np.uint32)
        sP, sN, sA, sT = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
        tk, tc, used = np.full((n, SLOTS), UNSET, np.uint32), np.zeros((n, SLOTS), np.uint32), np.zeros(n, np.int64)
        slot = np.arange(SLOTS)[None, :]
        distinct = [set() for _ in range(n)]
        for f in fs:                                                      # one add per sample, in sample order
            h = f["hit"]
            n_hit = n_hit + h.astype(np.uint32)
            sP = np.where(col(h), sP + f["P"], sP)
            sT = np.where(h, sT + f["t"], sT)
            sN = np.where(col(h), sN + f["N"], sN)
            sA = sA + f["a"]
            k = f["inst"] if key == "instance" else f["mat"]
            same = (slot < col(used)) & (tk == col(k))
            tc = tc + same.astype(np.uint32)
            fresh = np.flatnonzero(~same.any(axis=1) & (used < SLOTS))
            tk[fresh, used[fresh]] = k[fresh]
            tc[fresh, used[fresh]] = 1
            used[fresh] += 1
            for i, kk in enumerate(k):
                distinct[i].add(int(kk))
        for arr in (sP, sN, sA, sT):
            assert arr.dtype == np.float32
        order = np.argsort(-tc.astype(np.int64), axis=1, kind="stable")[:, :RANKS]      # count descending, first appearance on ties
        rc = np.take_along_axis(tc, order, axis=1)
        rk = np.where(rc > 0, np.take_along_axis(tk, order, axis=1), U(UNSET)).astype(np.uint32)
        any_hit = n_hit > 0
        zero = np.zeros(n, np.float32)
        with np.errstate(all="ignore"):
            nh, ns = n_hit.astype(np.float32), F(samples)
            pos = np.where(col(any_hit), np.column_stack([sP / col(nh), sT / nh]), np.column_stack([zero, zero, zero, np.full(n, 1e30, np.float32)]))
            nrm = np.where(col(any_hit), np.column_stack([sN / col(nh), zero]), F(0.0))
            alb = np.column_stack([sA / ns, nh / ns])
        f0 = fs[0]
        ids = np.column_stack([f0["inst"], f0["prim"], f0["mat"], n_hit]).astype(np.uint32)
        shape = (len(self.rows), self.width, 4)
        planes = {"position": pos.astype(np.float32).reshape(shape), "normal": nrm.astype(np.float32).reshape(shape),
                  "albedo": alb.astype(np.float32).reshape(shape), "id": ids.reshape(shape),
                  "matte_key": rk.reshape(shape), "matte_count": rc.astype(np.uint32).reshape(shape)}
        # a tie the ranking has to break: two equal counts next to each other among the ranks that go out, or at their edge
        by_count = -np.sort(-tc.astype(np.int64), axis=1)
        tied = ((by_count[:, :RANKS] == by_count[:, 1:RANKS + 1]) & (by_count[:, 1:RANKS + 1] > 0)).any(axis=1)
        info = {"n_hit": n_hit, "distinct": np.array([len(s) for s in distinct]), "tied": tied, "features": fs}
        return planes, info


def assert_planes_equal(got, want, what):
    for name in PLANES:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what} {name}: {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert len(bad) == 0, (f"{what}: plane {name}: {len(bad)} words differ, first (row, x, channel) {bad[:4].tolist()}: "
                               f"got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


@pytest.fixture(scope="module")
def indoor(oracle_scene):
    """The bundled scene's default 100 x 37 view (shared; its frames are traced once)."""
    return Expected(oracle_scene, oracle_scene.camera_ubo(W, H), W, range(H))


# ---- 0. the restated sampler is the oracle's ----------------------------------

def test_restated_rays_are_the_oracles(oracle_scene, indoor):
    assert np.frombuffer(indoor.ubo, np.float32)[31] == F(0.5)           # the bundled camera has a lens
    assert len(SPREAD) >= 64
    assert_rays_pinned(oracle_scene, indoor.ubo, W, H, 3, SPREAD)
    assert_rays_pinned(oracle_scene, indoor.ubo, W, H, 0, SPREAD[::8])


# ---- 1. bundled view ----------------------------------------------------------

def test_indoor_planes_bitexact(product_scene, indoor):
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        for first in (0, 7):
            for samples in (1, 5, 16):
                want, info = indoor.planes(samples, first)
                got = r.aov_sampled(samples, first)
                assert_planes_equal(got, want, f"indoor, samples {samples}, first_sample {first}")
                if samples == 1:
                    # one sample: the planes are that sample's features themselves (0.0f + x, then x / 1.0f:
                    # x word for word, but for a -0.0f component, which the sum turns into +0.0f)
                    f, m = info["features"][0], info["features"][0]["hit"].reshape(H, W)
                    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), (F(0.0) + b).view(np.uint32))
                    assert same(got["position"][m][:, :3], f["P"][f["hit"]]) and same(got["position"][m][:, 3], f["t"][f["hit"]])
                    assert same(got["normal"][m][:, :3], f["N"][f["hit"]])
                    assert same(got["albedo"][..., :3].reshape(-1, 3), f["a"])
                    assert np.array_equal(got["matte_key"][..., 0].ravel(), f["inst"]) and (got["matte_count"][..., 0] == 1).all()
                    assert (got["matte_count"][..., 1:] == 0).all() and (got["matte_key"][..., 1:] == UNSET).all()
                if samples == 16:
                    # the frame exercises mixed pixels (oracle side).  The bundled view is a closed room: the
                    # oracle finds no sample that misses, so 0 < nHit < samples is asserted where it can
                    # hold, on the moved camera of test_misses_after_set_camera
                    assert (info["n_hit"] == samples).all()
                    assert (info["distinct"] >= 2).sum() >= 100, "too few pixels see two keys"
                    assert_planes_equal(r.aov_sampled(samples, first), got, "second read (the cached planes)")
        assert r.debug_aov_sampled_time() > 0.0
        want, _ = indoor.planes(5, 0, "material")
        assert_planes_equal(r.aov_sampled(5, 0, "material"), want, "indoor, material keys")
    finally:
        r.close()


# ---- 2. lens and wrap-around ----------------------------------------------------

def test_no_lens_and_seed_wraparound(product_scene, indoor):
    r = surf_amd.Renderer(product_scene, W, H)
    o = oracle.OracleScene()
    try:
        # a frame index near 2^32 / 1799: the seed sum wraps within the 16 samples
        first = (1 << 32) // 1799 - 5
        assert (W * H + 1799 * (first + 15)) >= (1 << 32) > 1799 * first
        assert_rays_pinned(o, indoor.ubo, W, H, first + 9, SPREAD[::8])
        exp = Expected(o, indoor.ubo, W, range(H))
        assert_planes_equal(r.aov_sampled(16, first), exp.planes(16, first)[0], "the bundled lens, wrapping seeds")
        # defocus angle 0: no disk draw
        o.set_view(defocus=0.0)
        ubo = o.camera_ubo(W, H)
        assert np.frombuffer(ubo, np.float32)[31] == F(0.0)
        assert_rays_pinned(o, ubo, W, H, 2, SPREAD[::4])
        pin = Expected(o, ubo, W, range(H))
        r.set_camera(ubo)
        assert_planes_equal(r.aov_sampled(5, 0), pin.planes(5, 0)[0], "pinhole camera")
        assert not np.array_equal(pin.planes(5, 0)[0]["position"], indoor.planes(5, 0)[0]["position"])
    finally:
        o.close()
        r.close()


# ---- 3. misses, through set_camera (the cache is dropped) -----------------------

def test_misses_after_set_camera(oracle_scene, product_scene, indoor):
    ubo = np.frombuffer(indoor.ubo, np.float32).copy()
    shift = np.array([0.0, 6.0, -12.0], np.float32)
    ubo[0:3] = ubo[0:3] + shift              # position
    ubo[16:19] = ubo[16:19] + shift          # first_pixel
    moved = ubo.tobytes()
    centre_hit = oracle_scene.trace_closest(*centre_rays(moved, W, range(H)))[3] != UNSET
    assert 0.3 <= 1.0 - centre_hit.mean() <= 0.8, f"{1.0 - centre_hit.mean():.3f} of the centre rays miss"
    samples = 5
    want, info = Expected(oracle_scene, moved, W, range(H)).planes(samples)
    none, part = info["n_hit"] == 0, (info["n_hit"] > 0) & (info["n_hit"] < samples)
    assert none.sum() > 100 and part.sum() >= 50, "the view lacks all-miss or partly covered pixels (0 < nHit < samples)"
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        before = r.aov_sampled(samples)      # default camera: fills the cache
        assert_planes_equal(before, indoor.planes(samples)[0], "default camera")
        r.set_camera(moved)
        got = r.aov_sampled(samples)
        assert_planes_equal(got, want, "moved camera")
        m = none.reshape(H, W)
        assert (got["albedo"][m][:, 3] == 0.0).all() and (got["position"][m][:, 3] == F(1e30)).all()
        assert (got["id"][m] == np.array([UNSET, UNSET, UNSET, 0], np.uint32)).all()
        assert (got["matte_key"][m] == UNSET).all() and (got["matte_count"][m] == np.array([samples, 0, 0, 0], np.uint32)).all()
        pm = part.reshape(H, W)
        assert ((got["albedo"][pm][:, 3] > 0.0) & (got["albedo"][pm][:, 3] < 1.0)).all()
        cover = surf_amd.matte_coverage(got["matte_key"], got["matte_count"], surf_amd.MATTE_MISS, samples)
        assert np.array_equal(cover, (F(samples) - info["n_hit"].astype(np.float32)).reshape(H, W) / F(samples))
    finally:
        r.close()


# ---- 4. global tables and the two-level lane walk --------------------------------

def test_global_tables_planes_bitexact():
    """Variant 3: 91 instances, so the trace and shading tables are read from global memory."""
    o = oracle.OracleScene(variant=3)
    p = surf_amd.Scene.indoor(variant=3)
    try:
        assert o.instance_count() > 64
        want, info = Expected(o, o.camera_ubo(W, H), W, range(H)).planes(5, 1)
        assert any(((f["inst"] >= 64) & f["hit"]).any() for f in info["features"]), "no sample sees an instance past the LDS table size"
        r = surf_amd.Renderer(p, W, H)
        assert_planes_equal(r.aov_sampled(5, 1), want, "variant 3 (global tables)")
        r.close()
    finally:
        o.close()
        p.close()


def test_two_level_lane_walk(indoor, monkeypatch):
    """The laneW kernel variant (two-level records, forced on the bundled scene)."""
    monkeypatch.setenv("SURF_LANEW", "1")
    p = surf_amd.Scene.indoor()
    try:
        r = surf_amd.Renderer(p, W, H)
        assert_planes_equal(r.aov_sampled(5, 0), indoor.planes(5, 0)[0], "indoor, two-level lane walk")
        r.close()
    finally:
        p.close()


# ---- 5. the matte table's limits ---------------------------------------------------

MATTE_W, MATTE_H = 4, 3
MATTE_VIEW = dict(pos=(0.0, 4.0, -9.5), target=(0.0, 3.0, 0.0), fov_y=100.0)


def test_matte_table_overflow_and_ties():
    """Variant 3 at a tiny frame, from the front wall with a wide lens: a pixel spans many of the 91
    instances, so its table overflows (the oracle counts up to 14 instances in a pixel; at 8 x 6
    from the default view it counts 5, so the camera is moved back and the frame shrunk).  The
    scene has 8 materials, so only the instance keys can overflow; both keys have ties."""
    o = oracle.OracleScene(variant=3)
    p = surf_amd.Scene.indoor(variant=3)
    try:
        o.set_view(**MATTE_VIEW)
        ubo = o.camera_ubo(MATTE_W, MATTE_H)
        exp = Expected(o, ubo, MATTE_W, range(MATTE_H))
        r = surf_amd.Renderer(p, MATTE_W, MATTE_H)
        r.set_camera(ubo)
        for key in surf_amd.MATTE_KEYS:
            want, info = exp.planes(64, 0, key)
            if key == "instance":
                assert (info["distinct"] > SLOTS).any(), f"no pixel has more than {SLOTS} keys (most: {info['distinct'].max()})"
            assert info["tied"].any(), "no pixel has two keys of one count"
            got = r.aov_sampled(64, 0, key)
            assert_planes_equal(got, want, f"variant 3, {MATTE_W} x {MATTE_H}, 64 samples, {key} keys")
            assert (got["matte_count"].sum(axis=2) <= 64).all()
        r.close()
    finally:
        o.close()
        p.close()


# ---- 6. other paths ------------------------------------------------------------------

def test_row_shards_assemble_to_the_frame(product_scene, indoor):
    specs = [surf_amd.ShardSpec(k, 3, 2) for k in range(3)]          # 19 row blocks, the last a single row
    want = indoor.planes(5, 7)[0]
    parts = []
    for s in specs:
        r = surf_amd.Renderer(product_scene, W, H, shard=s)
        parts.append(r.aov_sampled(5, 7))
        r.close()
    assert sorted(len(p["id"]) for p in parts) == [12, 12, 13]
    for name in PLANES:
        # assemble_shards places float32 rows: the integer planes travel as float32 views of their bits
        got = surf_amd.assemble_shards(W, H, [p[name].view(np.float32) for p in parts], specs)
        assert np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name


def test_planes_follow_instance_update():
    o = oracle.OracleScene()
    p = surf_amd.Scene.indoor()
    try:
        ubo = o.camera_ubo(W, H)
        r = surf_amd.Renderer(p, W, H)
        before = r.aov_sampled(5)
        assert_planes_equal(before, Expected(o, ubo, W, range(H)).planes(5)[0], "before the update")
        o.update(0.5)
        p.update(0.5)
        r.update_instances(p)
        want = Expected(o, ubo, W, range(H)).planes(5)[0]
        got = r.aov_sampled(5)
        assert_planes_equal(got, want, "after update(0.5)")
        assert not np.array_equal(got["position"], before["position"]), "the update moved nothing in view"
        r.close()
    finally:
        o.close()
        p.close()


def test_read_is_neutral_to_the_sample_stream(product_scene):
    w, h = 32, 24
    out = []
    for read in (True, False):
        r = surf_amd.Renderer(product_scene, w, h)
        r.render(2, 0)
        if read:
            planes = r.aov_sampled(4, 0)
            assert (planes["id"][..., 3] > 0).any()
        r.render(2, 2)
        out.append((r.accumulator(), r.stats()))
        r.close()
    (acc_a, st_a), (acc_b, st_b) = out
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc", "samples"):
        assert st_a[k] == st_b[k], k
    assert st_a["samples"] == 4 * w * h


def test_status_codes_and_device_copy(product_scene, indoor):
    lib = surf_amd.load()
    buf = np.zeros((8, 8, 4), np.float32)
    q = surf_amd.aov_sampled_params()
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        assert lib.surf_read_aov_sampled(h, C.byref(q), 0, buf.ctypes.data) == -4     # SURF_ERR_NO_SCENE: nothing uploaded
        assert lib.surf_read_aov_sampled(h, C.byref(q), 6, buf.ctypes.data) == -1     # SURF_ERR_INVALID: planes are 0..5
        assert lib.surf_read_aov_sampled(h, C.byref(q), -1, buf.ctypes.data) == -1
        assert lib.surf_read_aov_sampled(h, C.byref(q), 0, None) == -1
        assert lib.surf_read_aov_sampled(h, None, 0, buf.ctypes.data) == -1
        assert lib.surf_copy_aov_sampled_device(h, C.byref(q), 0, None) == -1
        for bad in (surf_amd.AovSampledParams(0, 0, 0, 0), surf_amd.AovSampledParams(65, 0, 0, 0),
                    surf_amd.AovSampledParams(16, 0, 2, 0), surf_amd.AovSampledParams(16, 0, 0, 1)):
            assert lib.surf_read_aov_sampled(h, C.byref(bad), 0, buf.ctypes.data) == -1
            assert lib.surf_set_filter_guides_sampled(h, C.byref(bad)) == -1
        g, n = C.c_int(), C.c_uint32()
        assert lib.surf_set_filter_guides_sampled(h, C.byref(surf_amd.AovSampledParams(64, 3, 1, 0))) == 0
        assert lib.surf_get_filter_guides(h, C.byref(g), C.byref(n)) == 0 and (g.value, n.value) == (2, 64)
        assert lib.surf_set_filter_guides(h, 2, 8) == -1                                  # mode 2 is not set through this call
        assert lib.surf_get_filter_guides(h, C.byref(g), C.byref(n)) == 0 and (g.value, n.value) == (2, 64)
        assert lib.surf_set_filter_guides(h, 0, 8) == 0
        assert lib.surf_get_filter_guides(h, C.byref(g), C.byref(n)) == 0 and (g.value, n.value) == (0, 8)
    finally:
        lib.surf_destroy(h)
    # the HIP runtime the library itself runs on (already mapped into this process)
    with open("/proc/self/maps") as maps:
        hip_path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    hip = C.CDLL(hip_path)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], \
        [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    r = surf_amd.Renderer(product_scene, W, H)
    dev = C.c_void_p()
    try:
        want = indoor.planes(5, 7)[0]
        assert hip.hipMalloc(C.byref(dev), W * H * 16) == 0
        for k, name in enumerate(PLANES):
            r.copy_aov_sampled_to(k, dev.value, samples=5, first_sample=7)
            got = np.zeros((H, W, 4), np.uint32)
            assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0   # hipMemcpyDeviceToHost
            assert np.array_equal(got, want[name].view(np.uint32)), name
    finally:
        if dev.value:
            hip.hipFree(dev)
        r.close()


# ---- 7. the sampled planes as filter guides -----------------------------------------------

def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_guides_switch(product_scene):
    spp = 4
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert r.filter_guides() == ("first_hit", 8)
        r.set_sample_squares(True)
        r.set_sample_buckets(4)
        r.render(spp, 0)
        acc, sq = r.accumulator(), r.sample_squares()
        h0, h1 = surf_amd.bucket_halves(r.sample_buckets())
        first, sampled = r.aov(), r.aov_sampled(spp, 0)
        assert not bits_equal(first["normal"], sampled["normal"])
        before = (r.denoise(), r.denoise_sampled(), r.denoise_regress())
        assert bits_equal(before[0], r.denoise_image(acc, first))
        r.set_filter_guides("sampled", samples=spp, first_sample=0)
        assert r.filter_guides() == ("sampled", spp)
        got = r.denoise()
        assert bits_equal(got, r.denoise_image(acc, sampled)), "surf_denoise with the sampled guides is not its image form on the sampled planes"
        assert not bits_equal(got, before[0]), "the sampled guides change nothing"
        assert bits_equal(r.denoise_sampled(), r.denoise_sampled_image(acc, sq, sampled)[0])
        want = r.denoise_regress_image(h0, h1, sampled)
        got = r.denoise_regress()
        assert bits_equal(got[0], want[0]) and bits_equal(got[1], want[1])
        # other params: the guides are computed again
        r.set_filter_guides("sampled", samples=2, first_sample=1)
        assert r.filter_guides() == ("sampled", 2)
        assert bits_equal(r.denoise(), r.denoise_image(acc, r.aov_sampled(2, 1)))
        r.set_filter_guides("first_hit")
        assert r.filter_guides() == ("first_hit", 8)
        after = (r.denoise(), r.denoise_sampled(), r.denoise_regress())
        assert bits_equal(after[0], before[0]) and bits_equal(after[1], before[1])
        assert bits_equal(after[2][0], before[2][0]) and bits_equal(after[2][1], before[2][1])
    finally:
        r.close()


# ---- 8. the C++ API and the example ------------------------------------------------------

def read_pfm(path):
    blob = open(path, "rb").read()
    magic, dims, scale, data = blob.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    assert magic == b"PF" and scale == b"-1.0"
    return np.frombuffer(data, "<f4").reshape(h, w, 3)[::-1]         # rows bottom to top in the file


def test_cpp_example_matches_python(product_scene, tmp_path):
    w, h, samples = 64, 48, 6
    exe = os.path.join(surf_amd._PKG, "build", "render_aov")
    prefix = str(tmp_path / "aov")
    # the trailing arguments are MAX_LINKS, then SAMPLES
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(w), str(h), prefix, "8", str(samples)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = surf_amd.Renderer(product_scene, w, h)
    want, first = r.aov_sampled(samples), r.aov()
    r.close()
    for name in ("position", "normal", "albedo"):
        pfm = read_pfm(f"{prefix}_sampled_{name}.pfm")
        assert np.array_equal(np.ascontiguousarray(pfm).view(np.uint32), np.ascontiguousarray(want[name][..., :3]).view(np.uint32)), name
    raw = np.fromfile(prefix + "_matte.bin", np.uint32)
    assert raw.size == 2 * w * h * 4
    raw = raw.reshape(2, h, w, 4)
    assert np.array_equal(raw[0], want["matte_key"]) and np.array_equal(raw[1], want["matte_count"])
    # the first-hit outputs are still written, and are what they were
    planes = np.fromfile(prefix + "_planes.bin", np.uint32).reshape(4, h, w, 4)
    for k, name in enumerate(surf_amd.AOV_PLANES):
        assert np.array_equal(planes[k], first[name].view(np.uint32)), name
