"""Ray-traced ambient occlusion and bent normals (surf_read_ao / Renderer.ao())
against the CPU oracle plus numpy.

Bar: bit-exact, planes compared as uint32 words.  The expected planes never
come from the code under test:
  * P, N and valid are the oracle-side restatement of the source planes --
    tests/test_gpu_aov.py's expected_planes (centre rays, trace_closest, the
    normal arithmetic) for the first-hit source, tests/test_gpu_aov_chain.py's
    chain_planes for the chain source -- and are asserted once to equal
    Renderer.aov() word for word;
  * the seeds (initSeed of the salted pixel-and-sample index, xorshift32), the
    cosine-weighted direction and the origin offset are explicit float32 numpy
    steps, the trigonometry surf_ref_sinf / surf_ref_cosf;
  * the verdicts are oracle.trace_any's;
  * the bent-normal sum runs in sample order, one add per unoccluded sample.

The direction's retry (while R.N == 0) cannot be provoked with real seeds: a
unit N gives R.N = dir.z up to rounding, and dir.z = sqrt(1 - r0) is 0 only for
r0 == 1, which (float)u32 * 2^-32 reaches for 128 of 2^32 states while the
other two terms would have to cancel exactly.  The restatement carries the loop
anyway; no hook forces it.

Frames are 100 x 37 (3,700 pixels: a partial last block, a width that is no
multiple of any group size) unless said otherwise.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import surf_amd
from test_gpu_aov import UNSET, W, H, expected_planes, read_pfm
from test_gpu_aov_chain import chain_planes

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
SALT = U(0x5AD0CC1D)
K_2PI = F(6.28318530717958647692528)
PLANES = surf_amd.AO_PLANES


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


# ---- the pass, restated (numpy uint32 / float32) ------------------------------

def wang_hash(s):
    s = (s ^ U(61)) ^ (s >> U(16))
    s = s * U(9)
    s = s ^ (s >> U(4))
    s = s * U(0x27d4eb2d)
    return s ^ (s >> U(15))


def init_seed(s):
    return wang_hash((s + U(1)) * U(0x11))


def rnd_f(s):
    """(rndF, next state): xorshift32, then (float)state * 2^-32."""
    s = s ^ (s << U(13))
    s = s ^ (s >> U(17))
    s = s ^ (s << U(5))
    return s.astype(np.float32) * F(2.3283064365387e-10), s


def ref_trig(theta):
    lib = surf_amd.load()
    sn = np.fromiter((lib.surf_ref_sinf(float(t)) for t in theta), np.float32, len(theta))
    cs = np.fromiter((lib.surf_ref_cosf(float(t)) for t in theta), np.float32, len(theta))
    return sn, cs


def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def cosine_try(seed, n):
    """One try of the render's cosine-weighted direction about n: (R, next state, accepted)."""
    col = lambda a: a[:, None]
    r0, seed = rnd_f(seed)
    r1, seed = rnd_f(seed)
    r = np.sqrt(r0)
    theta = K_2PI * r1
    sn, cs = ref_trig(theta)
    dx, dy, dz = r * cs, r * sn, np.sqrt(F(1.0) - r0)
    x_max = F(1.0) - F(1e-5)
    tmp = np.where(col(np.abs(n[:, 0]) > x_max), np.array([0, 1, 0], np.float32), np.array([1, 0, 0], np.float32))
    c = cross(n, tmp)
    b = c * col(F(1.0) / np.sqrt(dot(c, c)))
    t = cross(b, n)
    out = (col(dx) * t + col(dy) * b) + col(dz) * n
    for a in (out, theta, dz):
        assert a.dtype == np.float32
    return out, seed, ~(dot(out, n) == F(0.0))


def cosine_sample(seed, n):
    out = np.zeros_like(n)
    todo = np.ones(len(n), bool)
    while todo.any():
        idx = np.flatnonzero(todo)
        r, s, ok = cosine_try(seed[idx], n[idx])
        out[idx], seed[idx] = r, s
        todo[idx] = ~ok
    return out


def pixel_index(width, rows):
    rows = np.asarray(list(rows), np.uint32)
    with np.errstate(over="ignore"):
        return np.tile(np.arange(width, dtype=np.uint32), len(rows)) + np.repeat(rows, width) * U(width)


def ao_rays(src, width, rows, samples, first_sample=0, bias=1e-5):
    """(valid pixel indices, [(O, R) per sample]) from the source planes."""
    P = src["position"].reshape(-1, 4)[:, :3]
    N = src["normal"].reshape(-1, 4)[:, :3]
    idx = np.flatnonzero(src["albedo"].reshape(-1, 4)[:, 3] != F(0.0))
    p = pixel_index(width, rows)[idx]
    rays = []
    for s in range(samples):
        with np.errstate(over="ignore"):
            seed = init_seed((p + U(1799) * U((first_sample + s) & 0xFFFFFFFF)) ^ SALT)
        R = cosine_sample(seed.copy(), np.ascontiguousarray(N[idx]))
        O = P[idx] + F(bias) * R
        assert O.dtype == np.float32 and R.dtype == np.float32
        rays.append((O, R))
    return idx, rays


def ao_expected(osc, src, width, rows, samples, radius, first_sample=0, bias=1e-5):
    """(planes, info): the two planes as (len(rows), width, 4), and the oracle's verdicts."""
    idx, rays = ao_rays(src, width, rows, samples, first_sample, bias)
    n, m = len(rows) * width, len(idx)
    lo, hi, n_open = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint32)
    S = np.zeros((m, 3), np.float32)
    for s, (O, R) in enumerate(rays):                                  # one add per unoccluded sample, in sample order
        is_open = osc.trace_any(O, R, np.full(m, radius, np.float32)) == 0
        S = np.where(is_open[:, None], S + R, S)
        if s < 32:
            lo = lo | (is_open.astype(np.uint32) << U(s))
        else:
            hi = hi | (is_open.astype(np.uint32) << U(s - 32))
        n_open = n_open + is_open.astype(np.uint32)
    assert S.dtype == np.float32
    no = n_open.astype(np.float32)
    with np.errstate(all="ignore"):
        bent = np.where((n_open > 0)[:, None], S / no[:, None], F(0.0)).astype(np.float32)
    openness = np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1))
    openness[idx] = np.column_stack([bent, no / F(samples)])
    bits = np.zeros((n, 4), np.uint32)
    bits[idx] = np.column_stack([lo, hi, n_open, np.ones(m, np.uint32)])
    shape = (len(rows), width, 4)
    info = {"valid": idx, "n_open": n_open, "occluded_share": 1.0 - n_open.sum() / max(1, m * samples),
            "mixed_share": ((n_open > 0) & (n_open < samples)).mean() if m else 0.0, "rays": rays}
    return {"openness": openness.reshape(shape), "bits": bits.reshape(shape)}, info


def assert_planes_equal(got, want, what):
    for name in PLANES:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what} {name}: {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert len(bad) == 0, (f"{what}: plane {name}: {len(bad)} words differ, first (row, x, channel) {bad[:4].tolist()}: "
                               f"got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


def frozen(planes):
    for a in planes.values():
        a.setflags(write=False)
    return planes


class Indoor:
    """The bundled scene's default 100 x 37 view: its source planes and, per params, the expected
    planes -- computed once and shared, read only."""

    def __init__(self, osc):
        self.osc = osc
        self.ubo = osc.camera_ubo(W, H)
        self.first = frozen(expected_planes(osc, self.ubo, W, range(H))[0])
        self.cache = {}

    def planes(self, samples, radius, first_sample=0, bias=1e-5):
        key = (samples, radius, first_sample, bias)
        if key not in self.cache:
            planes, info = ao_expected(self.osc, self.first, W, range(H), samples, radius, first_sample, bias)
            self.cache[key] = (frozen(planes), info)
        return self.cache[key]


@pytest.fixture(scope="module")
def indoor(oracle_scene):
    return Indoor(oracle_scene)


# ---- 1. bundled view, 16 samples, radius 4.0 -----------------------------------

def test_indoor_planes_bitexact(product_scene, indoor):
    want, info = indoor.planes(16, 4.0)
    # the oracle's verdicts: the frame is no degenerate case
    assert 0.05 <= info["occluded_share"] <= 0.95, f"{info['occluded_share']:.3f} of the rays are occluded"
    assert info["mixed_share"] >= 0.25, f"{info['mixed_share']:.3f} of the pixels are mixed"
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        aov = r.aov()
        for name in ("position", "normal", "albedo"):                  # the restated P, N, valid are the product's
            assert np.array_equal(aov[name].view(np.uint32), indoor.first[name].view(np.uint32)), name
        got = r.ao(16, 4.0)
        assert got["openness"].dtype == np.float32 and got["bits"].dtype == np.uint32
        assert_planes_equal(got, want, "indoor, 16 samples, radius 4")
        assert_planes_equal(r.ao(16, 4.0), got, "second read (the cached planes)")
        assert r.debug_ao_time() > 0.0
        # what the planes say of themselves
        b = got["bits"].reshape(-1, 4)
        assert np.array_equal(b[:, 2], np.array([bin(int(l)).count("1") + bin(int(h)).count("1") for l, h in b[:, :2]], np.uint32))
        assert np.array_equal(got["openness"].reshape(-1, 4)[:, 3][b[:, 3] == 1], b[:, 2][b[:, 3] == 1].astype(np.float32) / F(16.0))
    finally:
        r.close()


# ---- 2. group sizes and seeds ----------------------------------------------------

@pytest.mark.parametrize("samples, first", [(1, 0), (2, 0), (64, 0xFFFFFFF0)])
def test_group_sizes_and_seed_wraparound(product_scene, indoor, samples, first):
    want, info = indoor.planes(samples, 4.0, first)
    assert 0.05 <= info["occluded_share"] <= 0.95
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        got = r.ao(samples, 4.0, first_sample=first)
        assert_planes_equal(got, want, f"indoor, {samples} samples from {first:#x}")
        if samples == 64:
            assert (got["bits"][..., 1] != 0).any(), "no sample past the 32nd is open"
    finally:
        r.close()


# ---- 3. radius limits ----------------------------------------------------------------

def test_radius_limits(product_scene, indoor):
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        # the bundled room is closed: rays without an end all meet something
        want, info = indoor.planes(16, 1e30)
        assert (info["n_open"] == 0).all(), "the oracle finds an open ray in the closed room"
        got = r.ao(16, 1e30)
        assert_planes_equal(got, want, "radius 1e30")
        assert (got["openness"] == 0.0).all() and not np.signbit(got["openness"]).any()
        assert (got["bits"] == np.array([0, 0, 0, 1], np.uint32)).all()
        # ... and hardly any ray of a millimetre does
        want, info = indoor.planes(16, 1e-3)
        assert info["occluded_share"] < 0.10, f"{info['occluded_share']:.3f} of the short rays are occluded"
        assert_planes_equal(r.ao(16, 1e-3), want, "radius 1e-3")
    finally:
        r.close()


# ---- 4. invalid pixels, through set_camera (the cache is dropped) -------------------

def test_misses_after_set_camera(oracle_scene, product_scene, indoor):
    samples = 16
    ubo = np.frombuffer(indoor.ubo, np.float32).copy()
    shift = np.array([0.0, 6.0, -12.0], np.float32)
    ubo[0:3] = ubo[0:3] + shift              # position
    ubo[16:19] = ubo[16:19] + shift          # first_pixel
    moved = ubo.tobytes()
    src = expected_planes(oracle_scene, moved, W, range(H))[0]
    valid = src["albedo"].reshape(-1, 4)[:, 3] != 0.0
    assert valid.sum() > 100 and (~valid).sum() > 100, "the view lacks hits or misses"
    # the ray map: a wave holds 64 / samples consecutive pixels; one of them holds both kinds
    per_wave = 64 // samples
    groups = np.pad(valid.astype(np.int8), (0, -len(valid) % per_wave), constant_values=-1).reshape(-1, per_wave)
    assert ((groups == 1).any(axis=1) & (groups == 0).any(axis=1)).any(), "no wave holds a hit and a miss pixel"
    want, info = ao_expected(oracle_scene, src, W, range(H), samples, 4.0)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert_planes_equal(r.ao(samples, 4.0), indoor.planes(samples, 4.0)[0], "default camera")
        r.set_camera(moved)
        got = r.ao(samples, 4.0)
        assert_planes_equal(got, want, "moved camera")
        miss = ~valid.reshape(H, W)
        assert (got["openness"][miss].view(np.uint32) == np.array([0, 0, 0, 1], np.float32).view(np.uint32)).all()
        assert (got["bits"][miss] == 0).all()
        assert (got["bits"][~miss][:, 3] == 1).all()
    finally:
        r.close()


# ---- 5. variants -------------------------------------------------------------------------

def test_global_tables_planes_bitexact():
    """Variant 3: 91 instances, so the trace tables are read from global memory."""
    o = oracle.OracleScene(variant=3)
    p = surf_amd.Scene.indoor(variant=3)
    try:
        assert o.instance_count() > 64
        src = expected_planes(o, o.camera_ubo(W, H), W, range(H))[0]
        want, info = ao_expected(o, src, W, range(H), 16, 4.0)
        assert 0.05 <= info["occluded_share"] <= 0.95 and info["mixed_share"] >= 0.25
        late = False
        for O, R in info["rays"]:
            t, _, _, inst, _ = o.trace_closest(O, R)
            late = late or bool(((inst != UNSET) & (inst >= 64) & (t < F(4.0))).any())
        assert late, "no ray meets an instance past the LDS table size"
        r = surf_amd.Renderer(p, W, H)
        assert_planes_equal(r.ao(16, 4.0), want, "variant 3 (global tables)")
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
        assert_planes_equal(r.ao(16, 4.0), indoor.planes(16, 4.0)[0], "indoor, two-level lane walk")
        r.close()
    finally:
        p.close()


@pytest.mark.parametrize("lane_map", ["0", "1"])
def test_both_lane_maps(product_scene, indoor, monkeypatch, lane_map):
    """SURF_AO_MAP: one lane per pixel (0) and one lane per ray (1, the default), each against the oracle."""
    monkeypatch.setenv("SURF_AO_MAP", lane_map)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        for samples in (4, 16):
            assert_planes_equal(r.ao(samples, 4.0), indoor.planes(samples, 4.0)[0], f"SURF_AO_MAP={lane_map}, {samples} samples")
    finally:
        r.close()


# ---- 6. the chain source --------------------------------------------------------------------

def test_chain_source(oracle_scene, product_scene, indoor):
    chain = chain_planes(oracle_scene, indoor.ubo, W, range(H), 8)[0]
    delta = chain["id"].reshape(-1, 4)[:, 3] >= 1                      # the chain followed a link: a mirror or glass first hit
    assert delta.sum() >= 60, "the view has no mirror or glass first hits"
    assert (chain["id"].reshape(-1, 4)[~delta] == indoor.first["id"].reshape(-1, 4)[~delta]).all()
    want = ao_expected(oracle_scene, chain, W, range(H), 16, 4.0)[0]
    first = indoor.planes(16, 4.0)[0]
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        got = r.ao(16, 4.0, source="chain", max_links=8)
        assert_planes_equal(got, want, "chain source, 8 links")
        same = (got["openness"].view(np.uint32) == first["openness"].view(np.uint32)).all(axis=2).ravel() & \
               (got["bits"] == first["bits"]).all(axis=2).ravel()
        assert same[~delta].all(), "a pixel whose first hit is no mirror or glass differs from the first-hit source"
        assert not same[delta].any(), "a pixel behind a mirror or glass equals the first-hit source"
        assert_planes_equal(r.ao(16, 4.0), first, "back to the first-hit source")
        assert_planes_equal(r.ao(16, 4.0, source="chain", max_links=0), first, "0 links are the first-hit planes")
    finally:
        r.close()


# ---- 7. other paths ---------------------------------------------------------------------------

def test_row_shards_assemble_to_the_frame(product_scene, indoor):
    specs = [surf_amd.ShardSpec(k, 3, 2) for k in range(3)]          # 19 row blocks, the last a single row
    want = indoor.planes(16, 4.0)[0]
    parts = []
    for s in specs:
        r = surf_amd.Renderer(product_scene, W, H, shard=s)
        parts.append(r.ao(16, 4.0))
        r.close()
    assert sorted(len(p["bits"]) for p in parts) == [12, 12, 13]
    for name in PLANES:
        # assemble_shards places float32 rows: the integer plane travels as a float32 view of its bits
        got = surf_amd.assemble_shards(W, H, [p[name].view(np.float32) for p in parts], specs)
        assert np.array_equal(got.view(np.uint32), want[name].view(np.uint32)), name


def test_planes_follow_instance_update():
    o = oracle.OracleScene()
    p = surf_amd.Scene.indoor()
    try:
        ubo = o.camera_ubo(W, H)
        r = surf_amd.Renderer(p, W, H)
        before = r.ao(8, 4.0)
        assert_planes_equal(before, ao_expected(o, expected_planes(o, ubo, W, range(H))[0], W, range(H), 8, 4.0)[0], "before the update")
        o.update(0.5)
        p.update(0.5)
        r.update_instances(p)
        got = r.ao(8, 4.0)
        assert_planes_equal(got, ao_expected(o, expected_planes(o, ubo, W, range(H))[0], W, range(H), 8, 4.0)[0], "after update(0.5)")
        assert not np.array_equal(got["bits"], before["bits"]), "the update moved nothing in view"
        r.close()
    finally:
        o.close()
        p.close()


def test_other_params_recompute(product_scene, indoor):
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        a = r.ao(16, 4.0)
        b = r.ao(16, 1.0)
        c = r.ao(16, 4.0, bias=1e-3)
        d = r.ao(16, 4.0, first_sample=16)
        assert_planes_equal(a, indoor.planes(16, 4.0)[0], "radius 4")
        assert_planes_equal(b, indoor.planes(16, 1.0)[0], "radius 1")
        assert_planes_equal(c, indoor.planes(16, 4.0, 0, 1e-3)[0], "bias 1e-3")
        assert_planes_equal(d, indoor.planes(16, 4.0, 16)[0], "first_sample 16")
        assert not np.array_equal(a["bits"], b["bits"]) and not np.array_equal(a["bits"], d["bits"])
        assert_planes_equal(r.ao(16, 4.0), a, "back to the first params")
    finally:
        r.close()


def test_read_is_neutral_to_the_sample_stream(product_scene):
    w, h = 32, 24
    out = []
    for read in (True, False):
        r = surf_amd.Renderer(product_scene, w, h)
        r.render(2, 0)
        if read:
            planes = r.ao(8, 4.0)
            assert (planes["bits"][..., 3] == 1).any()
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
    q = surf_amd.ao_params()
    zero2 = lambda: (C.c_uint32 * 2)(0, 0)
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        assert lib.surf_read_ao(h, C.byref(q), 0, buf.ctypes.data) == -4     # SURF_ERR_NO_SCENE: nothing uploaded
        assert lib.surf_read_ao(h, C.byref(q), 2, buf.ctypes.data) == -1     # SURF_ERR_INVALID: planes are 0..1
        assert lib.surf_read_ao(h, C.byref(q), -1, buf.ctypes.data) == -1
        assert lib.surf_read_ao(h, C.byref(q), 0, None) == -1
        assert lib.surf_read_ao(h, None, 0, buf.ctypes.data) == -1
        assert lib.surf_copy_ao_device(h, C.byref(q), 0, None) == -1
        inf, nan = float("inf"), float("nan")
        for bad in (surf_amd.AoParams(0, 0, 1.0, 1e-5, 0, 8, zero2()), surf_amd.AoParams(3, 0, 1.0, 1e-5, 0, 8, zero2()),
                    surf_amd.AoParams(128, 0, 1.0, 1e-5, 0, 8, zero2()), surf_amd.AoParams(16, 0, 0.0, 1e-5, 0, 8, zero2()),
                    surf_amd.AoParams(16, 0, -1.0, 1e-5, 0, 8, zero2()), surf_amd.AoParams(16, 0, nan, 1e-5, 0, 8, zero2()),
                    surf_amd.AoParams(16, 0, -inf, 1e-5, 0, 8, zero2()), surf_amd.AoParams(16, 0, 1.0, -1e-5, 0, 8, zero2()),
                    surf_amd.AoParams(16, 0, 1.0, nan, 0, 8, zero2()), surf_amd.AoParams(16, 0, 1.0, 1e-5, 2, 8, zero2()),
                    surf_amd.AoParams(16, 0, 1.0, 1e-5, 1, 17, zero2()), surf_amd.AoParams(16, 0, 1.0, 1e-5, 0, 8, (C.c_uint32 * 2)(0, 1))):
            assert lib.surf_read_ao(h, C.byref(bad), 0, buf.ctypes.data) == -1
        ms = C.c_float(-1.0)
        assert lib.surf_debug_ao_time(h, C.byref(ms)) == 0 and ms.value == 0.0       # 0 before the first launch
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
        want = indoor.planes(16, 4.0)[0]
        assert hip.hipMalloc(C.byref(dev), W * H * 16) == 0
        for k, name in enumerate(PLANES):
            r.copy_ao_to(k, dev.value, samples=16, radius=4.0)
            got = np.zeros((H, W, 4), np.uint32)
            assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0   # hipMemcpyDeviceToHost
            assert np.array_equal(got, want[name].view(np.uint32)), name
            assert np.array_equal(got, r.ao(16, 4.0)[name].view(np.uint32)), name
        # infinite radius and zero bias are in range
        assert (r.ao(16, float("inf"))["bits"][..., 2] == 0).all()
        assert r.ao(16, 4.0, bias=0.0)["bits"].shape == (H, W, 4)
    finally:
        if dev.value:
            hip.hipFree(dev)
        r.close()


def test_cpp_example_matches_python(product_scene, tmp_path):
    w, h, samples, radius = 64, 48, 8, 2.5
    exe = os.path.join(surf_amd._PKG, "build", "render_ao")
    prefix = str(tmp_path / "ao")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(w), str(h), str(samples), str(radius), prefix], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = surf_amd.Renderer(product_scene, w, h)
    want = r.ao(samples, radius)
    r.close()
    bent, grey = read_pfm(prefix + "_bent.pfm"), read_pfm(prefix + "_open.pfm")
    assert np.array_equal(np.ascontiguousarray(bent).view(np.uint32), np.ascontiguousarray(want["openness"][..., :3]).view(np.uint32))
    for k in range(3):
        assert np.array_equal(np.ascontiguousarray(grey[..., k]).view(np.uint32), np.ascontiguousarray(want["openness"][..., 3]).view(np.uint32))
    assert ((want["openness"][..., 3] > 0.0) & (want["openness"][..., 3] < 1.0)).any()
