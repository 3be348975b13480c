"""Leaf runs of the lane walk (traceScene / leafRun, SURF_LEAF_RUN): the room's
planes are taken per lane, each lane its own instances in TLAS order, instead
of every plane by the whole wave.  Bar: bit-exact against the CPU oracle, with
the switch off and on, in both trace modes -- t, u, v, instance, primitive of
the closest hit, the occlusion byte of any-hit, and a render's accumulator and
event counts.

The rays are chosen for what the per-lane walk could get wrong: neighbouring
lanes that meet different planes, two or three planes at equal distance (edges
and corners: the tie the oracle's instance order decides), rays inside a
plane, a wave none of whose lanes enters the run, and a wave with one lane in
it.  Scene variant 0 throughout.
"""
import numpy as np
import pytest

import oracle
import surf_amd

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
UNSET = 0xFFFFFFFF

# the room (examples/indoor_scene.hpp): floor, walls, ceiling as instances of plane.obj
LO = np.array([-10.0, -1.0, -10.0])
HI = np.array([10.0, 9.0, 10.0])
CAMERA = np.array([0.0, 0.0, -7.0], np.float32)
RED_SUZANNE = np.array([0.0, 0.0, -1.0], np.float32)      # instance 3
RED_SUZANNE_INST = 3


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def plane_boxes(pad):
    """World boxes of the six planes, each the room's box flattened onto one
    face and grown by `pad` (the upload pads by ~0.007: a smaller pad here makes
    the count below an underestimate)."""
    boxes = []
    for axis in range(3):
        for side in (LO, HI):
            lo, hi = LO.copy(), HI.copy()
            lo[axis] = hi[axis] = side[axis]
            boxes.append((lo - pad, hi + pad))
    return boxes


def boxes_in_range(o, d, depth, pad=0.005):
    """Per ray: how many plane boxes the instance cull's slab test admits within [0, depth)."""
    o = o.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rd = (np.float32(1.0) / d.astype(np.float32)).astype(np.float32)
        n = np.zeros(len(o), np.int32)
        for lo, hi in plane_boxes(pad):
            ta = ((lo.astype(np.float32) - o) * rd).astype(np.float32)
            tb = ((hi.astype(np.float32) - o) * rd).astype(np.float32)
            t0 = np.fmax(np.fmax(np.fmin(ta[:, 0], tb[:, 0]), np.fmin(ta[:, 1], tb[:, 1])), np.fmin(ta[:, 2], tb[:, 2]))
            t1 = np.fmin(np.fmin(np.fmax(ta[:, 0], tb[:, 0]), np.fmax(ta[:, 1], tb[:, 1])), np.fmax(ta[:, 2], tb[:, 2]))
            n += ~((t1 < t0) | (t1 < 0.0) | (t0 >= depth))
    return n


def edge_corner_rays(n=4096, seed=23):
    """Rays from interior points through points on the room's 12 edges and 8
    corners, shuffled so that one wave's lanes meet different planes."""
    rng = np.random.default_rng(seed)
    targets = []
    per_edge = (n - 8 * 32) // 12
    for axis in range(3):                      # the 4 edges that run along `axis`
        a, b = [k for k in range(3) if k != axis]
        for sa in (LO, HI):
            for sb in (LO, HI):
                p = np.zeros((per_edge, 3))
                p[:, axis] = rng.uniform(LO[axis], HI[axis], per_edge)
                p[:, a] = sa[a]
                p[:, b] = sb[b]
                targets.append(p)
    for cx in (LO, HI):
        for cy in (LO, HI):
            for cz in (LO, HI):
                targets.append(np.tile([cx[0], cy[1], cz[2]], (32, 1)))
    tg = np.concatenate(targets)
    tg = np.concatenate([tg, tg[: n - len(tg)]])
    src = rng.uniform(LO + 0.5, HI - 0.5, size=(n, 3))
    o = src.astype(np.float32)
    dv = (tg.astype(np.float32) - o).astype(np.float32)
    d = (dv / np.linalg.norm(dv, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
    perm = rng.permutation(n)
    return o[perm], d[perm]


def in_plane_rays(per_plane=64, seed=29):
    """Rays that start on a plane and run along it (one direction component exactly 0)."""
    rng = np.random.default_rng(seed)
    os_, ds_ = [], []
    for axis in range(3):
        for side in (LO, HI):
            o = rng.uniform(LO + 1.0, HI - 1.0, size=(per_plane, 3))
            o[:, axis] = side[axis]
            d = rng.normal(size=(per_plane, 3))
            d[:, axis] = 0.0
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            os_.append(o)
            ds_.append(d)
    return np.concatenate(os_).astype(np.float32), np.concatenate(ds_).astype(np.float32)


def suzanne_rays(n, seed=31):
    """n rays from the camera position at the red Suzanne's centre (a small spread around it)."""
    rng = np.random.default_rng(seed)
    tg = RED_SUZANNE + rng.uniform(-0.05, 0.05, size=(n, 3)).astype(np.float32)
    dv = (tg - CAMERA).astype(np.float32)
    d = (dv / np.linalg.norm(dv, axis=1, keepdims=True)).astype(np.float32)
    return np.tile(CAMERA, (n, 1)).astype(np.float32), d


@pytest.fixture(scope="module")
def ray_sets(oracle_scene):
    """The test rays, the oracle's closest hits of them and the any-hit cases
    built on those hits -- computed once, shared by every mode and switch."""
    eo, ed = edge_corner_rays()
    po, pd = in_plane_rays()
    o, d = np.concatenate([eo, po]), np.concatenate([ed, pd])
    cpu = oracle_scene.trace_closest(o, d)
    t, inst = cpu[0], cpu[3]
    depth = np.where(inst != UNSET, t, np.float32(1e30)).astype(np.float32)
    # the multi-turn path is certain to run: a quarter of the rays or more meet two or more plane boxes in range
    multi = (boxes_in_range(o, d, depth) >= 2).mean()
    assert multi >= 0.25, f"only {multi:.1%} of the rays meet two or more plane boxes"
    far = np.float32(np.inf)
    any_cases = []
    for tm in (depth, np.nextafter(depth, np.float32(0)), np.nextafter(depth, far)):
        tm = tm.astype(np.float32)
        any_cases.append((tm, oracle_scene.trace_any(o, d, tm)))
    assert (inst != UNSET).mean() > 0.5 and any(c.any() for _, c in any_cases) and not all(c.all() for _, c in any_cases)
    return o, d, cpu, any_cases


def _assert_records(gpu, cpu, what):
    for n, g, c in zip(["t", "u", "v", "inst", "prim"], gpu, cpu):
        bad = np.nonzero(g.view(np.uint32) != c.view(np.uint32))[0]
        assert len(bad) == 0, f"{what} {n}: {len(bad)} of {len(g)} differ, first {bad[:5]}"


@pytest.mark.parametrize("leaf_run", ["0", "1"], ids=["loop", "runs"])
@pytest.mark.parametrize("mode", [0, 1], ids=["lane", "wave"])
def test_edges_corners_in_plane_bitexact(ray_sets, product_scene, mode, leaf_run, monkeypatch):
    o, d, cpu, any_cases = ray_sets
    monkeypatch.setenv("SURF_LEAF_RUN", leaf_run)
    r = surf_amd.Renderer(product_scene, 64, 64)
    try:
        r.set_trace_mode(mode)
        _assert_records(r.trace_closest(o, d), cpu, f"mode {mode} switch {leaf_run}")
        for k, (tmax, occ) in enumerate(any_cases):
            g = r.trace_any(o, d, tmax)
            bad = np.nonzero(g != occ)[0]
            assert len(bad) == 0, f"mode {mode} switch {leaf_run} any-hit case {k}: {len(bad)} differ, first {bad[:5]}"
    finally:
        r.close()


@pytest.fixture(scope="module")
def mask_sets(oracle_scene):
    """A full wave and a wave plus one lane none of whose rays enters the run
    (their depth is short before it), and the latter with a single ray to a wall."""
    sets = []
    for n in (64, 65):
        o, d = suzanne_rays(n)
        cpu = oracle_scene.trace_closest(o, d)
        assert (cpu[3] == RED_SUZANNE_INST).all(), "a ray missed the red Suzanne"
        assert (boxes_in_range(o, d, cpu[0], pad=0.05) == 0).all(), "a ray meets a plane box before its hit"
        sets.append((o, d, cpu))
    o, d, _ = sets[1]
    o, d = o.copy(), d.copy()
    wall = (np.array([-10.0, 4.0, 0.5], np.float32) - CAMERA).astype(np.float32)
    d[37] = wall / np.linalg.norm(wall)
    cpu = oracle_scene.trace_closest(o, d)
    assert cpu[3][37] == 6 and (np.delete(cpu[3], 37) == RED_SUZANNE_INST).all()
    sets.append((o, d, cpu))
    return sets


@pytest.mark.parametrize("leaf_run", ["0", "1"], ids=["loop", "runs"])
@pytest.mark.parametrize("mode", [0, 1], ids=["lane", "wave"])
def test_empty_and_lone_masks_bitexact(mask_sets, oracle_scene, product_scene, mode, leaf_run, monkeypatch):
    monkeypatch.setenv("SURF_LEAF_RUN", leaf_run)
    r = surf_amd.Renderer(product_scene, 64, 64)
    try:
        r.set_trace_mode(mode)
        for k, (o, d, cpu) in enumerate(mask_sets):
            _assert_records(r.trace_closest(o, d), cpu, f"set {k} mode {mode} switch {leaf_run}")
            tmax = np.full(len(o), 1e30, np.float32)
            assert np.array_equal(r.trace_any(o, d, tmax), oracle_scene.trace_any(o, d, tmax)), f"set {k} any-hit"
    finally:
        r.close()


@pytest.fixture(scope="module")
def render_reference(oracle_scene):
    oracle.set_zero_cutoff(True)
    try:
        acc, cnt, _ = oracle_scene.render(64, 64, 4)
    finally:
        oracle.set_zero_cutoff(False)
    return acc, cnt


@pytest.mark.parametrize("leaf_run", ["0", "1"], ids=["loop", "runs"])
def test_render_through_drain_bitexact(render_reference, product_scene, leaf_run, monkeypatch):
    """64x64, 4 frames, wavefront phases then the staged drain with the partner-wave tail."""
    acc, cnt = render_reference
    monkeypatch.setenv("SURF_LEAF_RUN", leaf_run)
    monkeypatch.setenv("SURF_TAIL_PAIR", "1")
    r = surf_amd.Renderer(product_scene, 64, 64)
    try:
        r.set_tail_policy(0, 0, 16)
        r.set_tail_coop(60000)
        r.render(4, 0, 0)
        g = r.accumulator()
        st = r.stats()
    finally:
        r.close()
    bad = np.argwhere(g.view(np.uint32) != acc.view(np.uint32))
    assert len(bad) == 0, f"switch {leaf_run}: {len(bad)} accumulator words differ, first {bad[:4].tolist()}"
    for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc"):
        assert st[k] == cnt[k], (k, st[k], cnt[k])
