"""GPU parity on caller-built scenes: the scenes, ray sets and product-side
descriptor of tests/test_custom_scenes_host.py, traced and rendered by the HIP
path and by the oracle (OracleScene.custom).

They reach what the bundled room and its variants never do in the host
re-layout (csrc/host/scene_upload.hip) and the kernels behind it: the
instance cull box under anisotropic, sheared, mirrored, ill-conditioned and far
translated matrices, instanceRay's divide path (an f32 inverse whose row 3 is
inexact, w != 1, a projective row), root leaves of 1..200 triangles, child
leaves around kLeafInW (3, 4) and around packLeaf's 128 (127, 128, 130), leaf runs (a run of 32
continued, a run broken by a projective copy, the position and instance
limits), LDS and global tables, 16- and 32-bit stacks around 65,536 BLAS
nodes, a BLAS too deep for the wave engines and one too deep to upload,
zero-area and duplicate triangles, zero-extent boxes, coordinates of 1e18 and
1e-18, a NaN vertex, a staged and an unstaged emitter BLAS.

Bar: bit-exact, as tests/test_gpu_parity.py: hit records as uint32 words,
occlusion bytes, accumulator words and event counts.  The conditions that make
a scene worth a GPU run are asserted on the CPU in the host file.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import surf_amd
from test_custom_scenes_host import TRACED, F, case
from test_gpu_aov import W as AW, H as AH, assert_planes_equal, expected_planes
from test_gpu_parity import _assert_bitexact, _assert_counts

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
W, H, FRAMES = 32, 24, 3
FIELDS = ["t", "u", "v", "inst", "prim"]
SURF_ERR_INVALID, SURF_ERR_LIMIT = -1, -7
WAVE = [n for n in TRACED if n != "Ddeep"]            # stack <= 64: the one-ray-per-wave walk and both drains


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


@pytest.fixture(scope="module")
def traced():
    """name -> the oracle's answers on the scene's rays, once per module: closest
    hits of every ray, and the any-hit sets with their answers."""
    done = {}

    def get(name):
        if name not in done:
            c = case(name)
            o, d = c.all_rays()
            cpu = c.oracle.trace_closest(o, d)
            so, sd, dist, _ = c.rays["silhouette"]
            with np.errstate(all="ignore"):
                half = (F(0.5) * np.minimum(cpu[0], F(1e20)) + F(0.25)).astype(np.float32)
            anys = [(o, d, half), (o, d, np.full(len(o), 1e30, np.float32))]
            anys += [(so, sd, tm) for tm in (dist, np.nextafter(dist, F(0)), np.nextafter(dist, F(np.inf)))]
            done[name] = (o, d, cpu, [(a, b, tm, c.oracle.trace_any(a, b, tm)) for a, b, tm in anys])
        return done[name]
    return get


@pytest.fixture(scope="module")
def rendered():
    """name -> (radiance, counters) of the oracle's 32 x 24 x 3 render, once per
    module, with _render_both's cutoff handling; no path may pass 4096 segments
    (one that never ends must not reach a GPU)."""
    done = {}

    def get(name):
        if name not in done:
            o = case(name).oracle
            oracle.set_zero_cutoff(True)
            try:
                c2, cnt, _ = o.render(W, H, FRAMES)
            finally:
                oracle.set_zero_cutoff(False)
            assert cnt["max_segments"] <= 4096, f"{name}: longest path {cnt['max_segments']} segments"
            c, _, _ = o.render(W, H, FRAMES)
            assert np.array_equal(c.view(np.uint32), c2.view(np.uint32)), "cutoff changed the oracle's radiance"
            assert cnt["n_hit"] > 0 and (c[..., :3] > 0).any(), f"{name}: an empty picture"
            print(f"{name} {W}x{H}x{FRAMES}: rays {cnt['n_ext']} hits {cnt['n_hit']} shadow rays {cnt['n_shadow']} "
                  f"unoccluded {cnt['n_unocc']} longest path {cnt['max_segments']}")
            c.setflags(write=False)
            done[name] = (c, cnt)
        return done[name]
    return get


def assert_hits_equal(gpu, cpu, what):
    for n, g, c in zip(FIELDS, gpu, cpu):
        bad = np.nonzero(np.asarray(g).view(np.uint32) != np.asarray(c).view(np.uint32))[0]
        assert len(bad) == 0, f"{what} {n}: {len(bad)} of {len(g)} differ, first {bad[:5]}: gpu {np.asarray(g)[bad[:5]]} cpu {np.asarray(c)[bad[:5]]}"


def assert_traces(r, answers, what):
    o, d, cpu, anys = answers
    assert_hits_equal(r.trace_closest(o, d), cpu, what)
    for k, (ao, ad, tm, want) in enumerate(anys):
        got = r.trace_any(ao, ad, tm)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, f"{what} any-hit set {k}: {len(bad)} of {len(got)} differ, first {bad[:5]}"


# ---- 1. traces -----------------------------------------------------------------

@pytest.mark.parametrize("lanew", ["0", "1"], ids=["one-level-lane-walk", "two-level-lane-walk"])
@pytest.mark.parametrize("name", TRACED)
def test_traces_bitexact(traced, name, lanew, monkeypatch):
    """trace_closest and trace_any on every ray set, one ray per lane (mode 0) and
    one per wave (mode 1), with the lane walk over the one-level records and
    over the two-level ones (SURF_LANEW=1, read at upload).  Ddeep's stack of
    102 entries is past the wave walk's 64: surf_set_trace_mode(1) refuses it
    (waveEligible, surf_hip.hip) and mode 0 still answers."""
    monkeypatch.setenv("SURF_LANEW", lanew)
    c = case(name)
    r = surf_amd.Renderer(c.product(), W, H)
    try:
        assert r.stats()["stack_depth"] == sum(c.oracle.bvh_depths()) + 1
        sel = r.debug_kernel_selection()
        assert sel["lane_two_level"] == (lanew == "1"), sel                 # the switch took: the two-level records exist
        assert sel["wave_eligible"] == (name in WAVE) and sel["lds_tables"] == (c.geometry.n <= 64), sel
        assert sel["stack16"] == (lanew == "0" and len(c.geometry.blas_nodes) < 65536), sel
        assert_traces(r, traced(name), f"{name} mode 0 laneW={lanew}")
        if name in WAVE:
            r.set_trace_mode(1)
            assert_traces(r, traced(name), f"{name} mode 1 laneW={lanew}")
        else:
            with pytest.raises(surf_amd.SurfError) as e:
                r.set_trace_mode(1)
            assert e.value.code == SURF_ERR_INVALID
            assert_traces(r, traced(name), f"{name} mode 0 after the refusal")
    finally:
        r.close()


def test_too_deep_upload_is_refused_and_the_context_lives(traced):
    """Dtoo's stack of 122 entries is past kMaxStack = 120: surf_upload_scene
    returns SURF_ERR_LIMIT, the context has no scene, and the next upload on the
    same context traces as a fresh one."""
    lib = surf_amd.load()
    a, b, bad = case("B1"), case("A"), case("Dtoo")
    with pytest.raises(surf_amd.SurfError) as e:
        surf_amd.Renderer(bad.product(), W, H)
    assert e.value.code == SURF_ERR_LIMIT and "too deep" in str(e.value)
    r = surf_amd.Renderer(a.product(), W, H)
    try:
        p = bad.product()
        d = p.desc()
        assert lib.surf_upload_scene(r.handle, C.byref(d)) == SURF_ERR_LIMIT
        with pytest.raises(surf_amd.SurfError) as e:
            r.trace_closest(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
        assert e.value.code == -4                                   # SURF_ERR_NO_SCENE
        p = b.product()
        d = p.desc()
        assert lib.surf_upload_scene(r.handle, C.byref(d)) == 0
        assert_traces(r, traced("A"), "A after a refused upload")
    finally:
        r.close()


# ---- 2. renders ----------------------------------------------------------------

RENDERED = ["A", "A2", "B64", "B65", "Cnan", "E0", "E1", "L1", "L2", "L1c", "L2c"]
ENGINES = {"wavefront-to-end": ((1, 0, 0), 0), "pair-from-start": ((1 << 30, 0, 8), 1 << 30), "coop-from-start": ((1 << 30, 0, 8), 1 << 30)}
# The drains take what is in flight when a replay ends.  In the closed scenes (A, A2 inside the scale-1e3 sphere, B inside
# its enclosure, L1c and L2c inside the same sphere) paths live long enough for that (22 to 64 paths measured); under the
# open sky of Cnan, E, L1 and L2 no path passes 7 segments and nothing is ever left, so a drain run there would repeat
# the wavefront one.
DRAINED = ["A", "A2", "B64", "B65", "L1c", "L2c"]
RUNS = [(n, e) for n in RENDERED for e in ENGINES if e == "wavefront-to-end" or n in DRAINED]


def render(name, engine, monkeypatch, env=None):
    policy, coop = ENGINES[engine]
    monkeypatch.setenv("SURF_TAIL_PAIR", "0" if engine.startswith("coop") else "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = surf_amd.Renderer(case(name).product(), W, H, pool_capacity=None if engine.startswith("wavefront") else 64)
    try:
        r.set_tail_policy(*policy)
        r.set_tail_coop(coop)
        r.render(FRAMES, 0, 0)
        return r.accumulator(), r.stats(), r.debug_connect_staging(), r.debug_kernel_selection()
    finally:
        r.close()


@pytest.mark.parametrize("name,engine", RUNS, ids=[f"{n}-{e}" for n, e in RUNS])
def test_renders_bitexact(rendered, name, engine, monkeypatch):
    """32 x 24, 3 frames: k_shade to the end, and (DRAINED) the partner-wave and the
    one-path-per-wave drain from the first phase with a pool of 64 paths
    (test_scenario_bitexact's set-up).  L1 stages its emitters' one BLAS in LDS,
    L2 with two emitter BLASes must not."""
    c, cnt = rendered(name)
    g, st, staging, sel = render(name, engine, monkeypatch)
    # E0's 65,534 BLAS nodes take k_extend's 16-bit stack, E1's 65,536 cannot; 64 instances are the last in LDS
    assert sel["stack16"] == (len(case(name).geometry.blas_nodes) < 65536) and sel["lds_tables"] == (case(name).geometry.n <= 64), sel
    assert sel["stack16"] == (name != "E1") and sel["lds_tables"] == (name != "B65") and not sel["lane_two_level"], sel
    print(f"{name} {engine}: drain paths {st['tail_survivors']}, drain rays {st['n_ext'] - st['n_ext_wavefront']} of {st['n_ext']}, staging {staging}")
    if engine.startswith("wavefront"):
        assert st["tail_survivors"] == 0
    else:
        assert st["tail_survivors"] > 0, f"the {engine} drain did not run"
    if name in ("L1", "L1c"):
        assert staging[0] > 0 and staging[1] == 32, staging
    if name in ("L2", "L2c"):
        assert staging == (0, 0)
    assert np.all(g[..., 3] == FRAMES) and st["samples"] == W * H * FRAMES
    _assert_bitexact(g, c, f"{name}, {engine}")
    _assert_counts(st, cnt)


@pytest.mark.parametrize("name", ["E0", "E1"])
def test_node_count_sides_with_a_32_bit_stack(rendered, name, monkeypatch):
    """E0 (65,534 BLAS nodes) takes k_extend's 16-bit stack by default and E1
    (65,536) cannot; SURF_EXT_STACK16=0 gives both the 32-bit one."""
    c, cnt = rendered(name)
    g, st, _, sel = render(name, "wavefront-to-end", monkeypatch, {"SURF_EXT_STACK16": "0"})
    assert not sel["stack16"], sel
    _assert_bitexact(g, c, f"{name}, 32-bit stack")
    _assert_counts(st, cnt)


# ---- 3. re-upload ----------------------------------------------------------------

def test_update_instances_to_other_matrices(traced, rendered):
    """Scene A, then surf_update_instances with Aalt's instance, TLAS and light
    buffers: the same meshes and counts, other matrices (affine rows turned
    projective and back, an inexact inverse row turned exact).  Traces and a
    render equal the oracle's Aalt and a fresh upload of it."""
    a, b = case("A"), case("Aalt")
    c, cnt = rendered("Aalt")
    r = surf_amd.Renderer(a.product(), W, H)
    fresh = surf_amd.Renderer(b.product(), W, H)
    try:
        assert_traces(r, traced("A"), "A before the update")
        r.render(FRAMES, 0, 0)
        pb = b.product()
        r.update_instances(pb)
        for mode in (0, 1):
            r.set_trace_mode(mode)
            assert_traces(r, traced("Aalt"), f"Aalt after update_instances, mode {mode}")
        r.set_trace_mode(0)
        r.clear_accumulator()
        r.render(FRAMES, 0, 0)
        g = r.accumulator()
        fresh.render(FRAMES, 0, 0)
        _assert_bitexact(g, c, "Aalt after update_instances")
        assert np.array_equal(g.view(np.uint32), fresh.accumulator().view(np.uint32))
        _assert_counts(fresh.stats(), cnt)
    finally:
        r.close()
        fresh.close()


def test_update_instances_to_another_run_layout(traced, rendered):
    """B1 -> B2 -> B1 through surf_update_instances: the same meshes and counts, but
    the plane at TLAS position 28 turns projective and back, so the leaf runs
    change from 32 + 8 to 17 + 22 and back (test_each_scene_reaches_its_branch
    asserts the two layouts).  setKeys must recompute runHead / runMember: a
    stale mask would put the projective copy into a run, or leave position 28
    out of one.  Traces in both modes and a render after each update equal the
    oracle's and a fresh upload's."""
    r = surf_amd.Renderer(case("B1").product(), W, H)
    try:
        assert_traces(r, traced("B1"), "B1 before the update")
        for name in ("B2", "B1"):
            c, cnt = rendered(name)
            p = case(name).product()
            r.update_instances(p)
            for mode in (0, 1):
                r.set_trace_mode(mode)
                assert_traces(r, traced(name), f"{name} after update_instances, mode {mode}")
            r.set_trace_mode(0)
            r.clear_accumulator()
            r.render(FRAMES, 0, 0)
            g = r.accumulator()
            fresh = surf_amd.Renderer(p, W, H)
            try:
                fresh.render(FRAMES, 0, 0)
                _assert_bitexact(g, c, f"{name} after update_instances")
                assert np.array_equal(g.view(np.uint32), fresh.accumulator().view(np.uint32))
                _assert_counts(fresh.stats(), cnt)
            finally:
                fresh.close()
    finally:
        r.close()


# ---- 4. feature planes -----------------------------------------------------------

@pytest.mark.parametrize("name", ["A", "B1"])
def test_feature_planes_bitexact(name):
    """aov() position, normal, albedo and ids against test_gpu_aov's numpy
    restatement fed by the custom oracle scene."""
    c = case(name)
    ubo = c.oracle.camera_ubo(AW, AH)
    want, info = expected_planes(c.oracle, ubo, AW, range(AH))
    assert info["hit"].mean() > 0.5 and len(np.unique(want["id"][..., 0])) >= 5
    r = surf_amd.Renderer(c.product(), AW, AH)
    try:
        assert_planes_equal(r.aov(), want, f"{name} first hit")
    finally:
        r.close()
