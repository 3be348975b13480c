"""The shadow queue's order bins (SURF_SH_KEY, shadowKey in
csrc/device/wavefront_kernels.h): layout 0 = light x octant (16 bins), 1 = any
heavy box on the segment first (32), 2 = three heavy classes x light x x/z
quadrant, then light x octant (40).

The order a phase's shadow rays are traced in changes no result, so every
layout, the unordered queue and a queue whose regions overflow give the
oracle's accumulator bit for bit and its event counts; the key itself is
checked against a numpy restatement (surf_debug_shadow_keys), and stays below
the number of bins in use for every ray, whatever its numbers.
"""
import numpy as np
import pytest

import oracle
import surf_amd
from test_custom_scenes_host import GREY, LAMP, RED, SKY, ExportedScene, Rot, Sc, T, f32, octa, plane2
from test_gpu_parity import _assert_bitexact, _assert_counts

pytestmark = pytest.mark.gpu
BINS = {"0": 16, "1": 32, "2": 40}
W, H, FRAMES = 64, 36, 8
SW, SH, SFRAMES = 48, 27, 4


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def oracle_render(o, w, h, frames, first=0):
    """_render_both's oracle side: radiance without the zero-throughput cutoff, event counts with it."""
    c, _, _ = o.render(w, h, frames, first_frame=first)
    oracle.set_zero_cutoff(True)
    try:
        c2, cnt, _ = o.render(w, h, frames, first_frame=first)
    finally:
        oracle.set_zero_cutoff(False)
    assert np.array_equal(c.view(np.uint32), c2.view(np.uint32)), "cutoff changed the oracle's radiance"
    c.setflags(write=False)
    return c, cnt


@pytest.fixture(scope="module")
def expected(oracle_scene):
    return oracle_render(oracle_scene, W, H, FRAMES)


def gpu_render(scene, w, h, frames, first=0):
    r = surf_amd.Renderer(scene, w, h)
    try:
        r.render(frames, first, 0)
        return r.accumulator(), r.stats()
    finally:
        r.close()


@pytest.mark.parametrize("env", [{"SURF_SH_KEY": "0"}, {"SURF_SH_KEY": "1"}, {"SURF_SH_KEY": "2"}, {"SURF_SORT": "2"}],
                         ids=["key-0", "key-1", "key-2", "one-bin"])
def test_render_bitexact_under_every_layout(expected, product_scene, env, monkeypatch):
    """64 x 36, 8 frames, unbounded bounces; no ray overflows its bin's region at this size."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c, cnt = expected
    g, st = gpu_render(product_scene, W, H, FRAMES)
    _assert_bitexact(g, c, f"shadow order {env}")
    _assert_counts(st, cnt)
    assert st["n_shadow_overflow"] == 0


@pytest.mark.parametrize("key", ["1", "2"])
def test_overflow_region_bitexact(expected, product_scene, key, monkeypatch):
    """Regions of 256 slots: most of a phase's shadow rays take the overflow region."""
    monkeypatch.setenv("SURF_SH_KEY", key)
    monkeypatch.setenv("SURF_SH_REGION", "256")
    c, cnt = expected
    g, st = gpu_render(product_scene, W, H, FRAMES)
    print(f"key {key}: {st['n_shadow_overflow']} of {st['n_shadow']} shadow rays in the overflow region")
    assert 0 < st["n_shadow_overflow"] <= st["n_shadow"]
    _assert_bitexact(g, c, f"key {key}, regions of 256")
    _assert_counts(st, cnt)


# ---- the key against a restatement ---------------------------------------------------

def slabs(o, d, lo, hi):
    """Entry and exit of each ray's line in one box, in the arrays' own precision, as heavyMask computes them."""
    with np.errstate(all="ignore"):
        r = o.dtype.type(1) / d
        a, b = (lo - o) * r, (hi - o) * r
        t0 = np.maximum(np.maximum(np.minimum(a[:, 0], b[:, 0]), np.minimum(a[:, 1], b[:, 1])), np.minimum(a[:, 2], b[:, 2]))
        t1 = np.minimum(np.minimum(np.maximum(a[:, 0], b[:, 0]), np.maximum(a[:, 1], b[:, 1])), np.maximum(a[:, 2], b[:, 2]))
    return t0, t1


def restated_keys(o, d, tmax, light, lay, bins, dtype):
    o, d, tmax = o.astype(dtype), d.astype(dtype), tmax.astype(dtype)
    cell = np.zeros(len(o), np.int64)
    for a in range(3):
        cell |= (((o[:, a] - dtype(lay["cell_lo"][a])) * dtype(lay["cell_scale"][a])) >= 1).astype(np.int64) << a
    li = light.astype(np.int64) & 1
    base = li * 8 + cell
    if bins == 16:
        return base
    m = np.zeros(len(o), np.int64)
    for h, (lo, hi) in enumerate(zip(lay["heavy_lo"], lay["heavy_hi"])):
        t0, t1 = slabs(o, d, lo.astype(dtype), hi.astype(dtype))
        m |= ((t1 >= t0) & (t1 > 0) & (t0 < tmax)).astype(np.int64) << h
    if bins == 32:
        return np.where(m != 0, base, 16 + base)
    cls = np.where((m & (m - 1)) != 0, 0, np.where(m & 1, 1, 2))
    return np.where(m != 0, cls * 8 + li * 4 + (cell & 1) + ((cell >> 1) & 2), 24 + base)


def margin_rays(lay, want, seed):
    """Rays whose every comparison in the key has a margin of more than 1e-3
    relative (v_rcp_f32's one ulp cannot flip one): origin coordinates off the
    cells' mid planes, direction components off zero, and in each heavy box the
    slab entry t0 and exit t1 apart from each other, t1 apart from 0 and t0
    apart from tmax."""
    rng = np.random.default_rng(seed)
    n = 6 * want
    lo, hi = lay["heavy_lo"].astype(np.float64), lay["heavy_hi"].astype(np.float64)
    mid = lay["cell_lo"].astype(np.float64) + 1.0 / lay["cell_scale"].astype(np.float64)
    ext = 1.0 / lay["cell_scale"].astype(np.float64)
    o = mid + rng.uniform(-1.05, 1.05, (n, 3)) * ext
    # half of the rays aim at a point in a heavy box, so that every mask occurs
    box = rng.integers(0, len(lo), n)
    aim = np.where(rng.random(n)[:, None] < 0.5, lo[box] + rng.random((n, 3)) * (hi[box] - lo[box]),
                   mid + rng.uniform(-1.0, 1.0, (n, 3)) * ext)
    d = aim - o
    dist = np.linalg.norm(d, axis=1)
    d /= dist[:, None]
    tmax = dist * rng.choice([0.3, 0.9, 1.5, 4.0], n)
    o, d, tmax = o.astype(np.float32), d.astype(np.float32), tmax.astype(np.float32)
    o64, d64, t64 = o.astype(np.float64), d.astype(np.float64), tmax.astype(np.float64)
    ok = (np.abs(d64) > 1e-2).all(axis=1) & (np.abs(o64 - mid) > 2e-3 * ext).all(axis=1)
    for b in range(len(lo)):
        t0, t1 = slabs(o64, d64, lo[b], hi[b])
        big = np.maximum(np.maximum(np.abs(t0), np.abs(t1)), t64)
        ok &= (np.abs(t1 - t0) > 2e-3 * big) & (np.abs(t1) > 2e-3 * big) & (np.abs(t0 - t64) > 2e-3 * big)
    keep = np.nonzero(ok)[0][:want]
    assert len(keep) == want, f"only {len(keep)} of {n} rays have the margins"
    return o[keep], d[keep], tmax[keep], rng.integers(0, 6, want).astype(np.uint32)


def edge_rays(lay, seed):
    """Rays the margins exclude: zero direction components, tmax = 0, origins
    inside a heavy box and on its faces, segments ending on a face, infinite and
    NaN directions, origins and tmax."""
    rng = np.random.default_rng(seed)
    lo, hi = lay["heavy_lo"].astype(np.float64), lay["heavy_hi"].astype(np.float64)
    ctr, half = (lo[0] + hi[0]) / 2, (hi[0] - lo[0]) / 2
    n = 64
    inside = ctr + rng.uniform(-0.9, 0.9, (n, 3)) * half
    outside = ctr + np.array([0.0, 0.0, -3.0]) * half + rng.uniform(-0.5, 0.5, (n, 3)) * half
    on_face = inside.copy()
    on_face[:, 0] = hi[0][0]
    rnd = rng.normal(size=(n, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    axis = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], n)[:, None]
    plane = rnd.copy()
    plane[:, 1] = 0.0
    to_face = np.array([0.0, 0.0, 1.0]) * np.ones((n, 1))
    sets = [(inside, rnd, np.full(n, 1e30)), (inside, axis, np.full(n, 5.0)), (outside, axis, np.full(n, 1e30)),
            (outside, plane, np.full(n, 2.0)), (outside, rnd, np.zeros(n)), (on_face, axis, np.full(n, 1.0)),
            (outside, to_face, lo[0][2] - outside[:, 2]), (outside, to_face, hi[0][2] - outside[:, 2]),
            (outside, np.zeros((n, 3)), np.full(n, 1.0)), (outside, rnd * np.inf, np.full(n, 1.0)),
            (outside, np.full((n, 3), np.nan), np.full(n, 1.0)), (outside, rnd, np.full(n, np.nan)),
            (outside, rnd, np.full(n, np.inf)), (np.full((n, 3), np.nan), rnd, np.full(n, 1.0)),
            (np.full((n, 3), np.inf), rnd, np.full(n, 1.0)), (outside * 1e30, rnd, np.full(n, -1.0))]
    with np.errstate(all="ignore"):
        o = np.concatenate([s[0] for s in sets]).astype(np.float32)
        d = np.concatenate([s[1] for s in sets]).astype(np.float32)
        t = np.concatenate([s[2] for s in sets]).astype(np.float32)
    return o, d, t, rng.integers(0, 1 << 32, len(o), dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("key", ["0", "1", "2"])
def test_keys_match_the_restatement(product_scene, key, monkeypatch):
    monkeypatch.setenv("SURF_SH_KEY", key)
    r = surf_amd.Renderer(product_scene, 32, 24)
    try:
        _, bins, lay = r.debug_shadow_keys(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0))
        assert bins == BINS[key]
        assert len(lay["heavy_lo"]) == 3 and (lay["heavy_hi"] > lay["heavy_lo"]).all() and (lay["cell_scale"] > 0).all(), lay
        o, d, tmax, light = margin_rays(lay, 4000, 11)
        k32 = restated_keys(o, d, tmax, light, lay, bins, np.float32)
        k64 = restated_keys(o, d, tmax, light, lay, bins, np.float64)
        assert np.array_equal(k32, k64), "the margins do not separate the f32 and the f64 restatement"
        got, _, _ = r.debug_shadow_keys(o, d, tmax, light)
        used = len(np.unique(k32))
        print(f"key {key}: {used} of {bins} bins occur")
        assert used >= (bins * 3) // 4
        bad = np.nonzero(got.astype(np.int64) != k32)[0]
        assert len(bad) == 0, f"{len(bad)} of {len(got)} keys differ, first {bad[:5]}: gpu {got[bad[:5]]} restated {k32[bad[:5]]}"
        eo, ed, et, el = edge_rays(lay, 12)
        got, _, _ = r.debug_shadow_keys(eo, ed, et, el)
        assert (got < bins).all(), f"keys {np.unique(got[got >= bins])} index past the {bins} bins"
    finally:
        r.close()


def test_one_bin_without_a_shadow_order(product_scene, monkeypatch):
    monkeypatch.setenv("SURF_SORT", "2")
    monkeypatch.setenv("SURF_SH_KEY", "2")
    r = surf_amd.Renderer(product_scene, 32, 24)
    try:
        got, bins, lay = r.debug_shadow_keys(*edge_rays({"heavy_lo": np.zeros((1, 3)), "heavy_hi": np.ones((1, 3))}, 13))
        assert bins == 1 and (got == 0).all()
    finally:
        r.close()


# ---- scenes that move the heavy set ----------------------------------------------------

def planes_and_a_lamp():
    """A floor, a back wall and two side walls of two triangles each under a
    32-triangle lamp and the gradient sky: no BLAS reaches the 64 triangles of a
    heavy instance."""
    inst = [(0, 0, f32(T(0, -12, 0) @ Sc(90.0))),
            (0, 1, f32(T(0, 0, 40) @ Rot((1, 0, 0), -90) @ Sc(90.0))),
            (0, 0, f32(T(-40, 0, 0) @ Rot((0, 0, 1), -90) @ Sc(90.0))),
            (0, 1, f32(T(40, 0, 0) @ Rot((0, 0, 1), 90) @ Sc(90.0))),
            (1, 2, f32(T(0, 20, 0) @ Sc(5.0)))]
    view = {"pos": (0.0, 25.0, -95.0), "target": (0.0, 0.0, 0.0), "fov_y": 60.0, "focal": 95.0, "defocus": 0.5}
    return oracle.OracleScene.custom([plane2(), octa(1)], [GREY, RED, LAMP], inst, background=SKY, view=view)


def test_scene_without_heavy_instances_bitexact(monkeypatch):
    """nHeavy == 0: layout 2 puts every ray in its last 16 bins."""
    monkeypatch.setenv("SURF_SH_KEY", "2")
    o = planes_and_a_lamp()
    try:
        c, cnt = oracle_render(o, SW, SH, SFRAMES)
        assert cnt["n_shadow"] > 0 and cnt["n_unocc"] > 0 and (c[..., :3] > 0).any(), cnt
        p = ExportedScene(o)
        r = surf_amd.Renderer(p, SW, SH)
        try:
            rng = np.random.default_rng(5)
            d = rng.normal(size=(512, 3))
            got, bins, lay = r.debug_shadow_keys(rng.uniform(-50, 50, (512, 3)), d / np.linalg.norm(d, axis=1, keepdims=True),
                                                 rng.uniform(0, 200, 512), rng.integers(0, 4, 512))
            assert bins == 40 and len(lay["heavy_lo"]) == 0 and (got >= 24).all() and (got < 40).all()
            r.render(SFRAMES, 0, 0)
            g, st = r.accumulator(), r.stats()
        finally:
            r.close()
        _assert_bitexact(g, c, "planes and a lamp, key 2")
        _assert_counts(st, cnt)
    finally:
        o.close()


def test_moved_heavy_instance_bitexact(monkeypatch):
    """surf_update_instances after GPUScene::update has turned instance 3, a
    Suzanne: the key's boxes follow it (setKeys) and the render is the oracle's."""
    monkeypatch.setenv("SURF_SH_KEY", "2")
    o = oracle.OracleScene()
    p = surf_amd.Scene.indoor()
    try:
        r = surf_amd.Renderer(p, SW, SH)
        try:
            none = (np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0))
            before = r.debug_shadow_keys(*none)[2]
            o.update(0.7)
            p.update(0.7)
            r.update_instances(p)
            after = r.debug_shadow_keys(*none)[2]
            assert len(after["heavy_lo"]) == 3
            assert not (np.array_equal(before["heavy_lo"], after["heavy_lo"]) and np.array_equal(before["heavy_hi"], after["heavy_hi"]))
            r.render(SFRAMES, 4, 0)
            g, st = r.accumulator(), r.stats()
        finally:
            r.close()
        c, cnt = oracle_render(o, SW, SH, SFRAMES, first=4)
        _assert_bitexact(g, c, "bundled scene after the update, key 2")
        _assert_counts(st, cnt)
    finally:
        o.close()
        p.close()
