"""Planted paths on the GPU (Renderer.debug_trace_paths) against the oracle's
trace() from the same origins, directions and RNG states
(OracleScene.trace_paths): energy words, segment counts and final seeds, in
both modes -- mode 0 one path per lane (the lane walk, shadePath<false> and
the lane any-hit walk: what k_extend, k_shade and k_connect run), mode 1 one
path per wave (traceWave, shadePath<true>, the wave any-hit walk: what the
cooperative drains run).

The inputs and what they stand on are tests/test_planted_paths_host.py's:

  * the 128 seeds per surface whose second draw is r0 == 1.0f, from
    (0.5, 2, 0.3) toward the floor, a side wall, the back wall and the ceiling:
    the retry of the cosine sample, which no render draws.  shadePath<true>
    forms the light sample from the state after the first try and must form it
    again after a retry; cosineSample's loop in k_shade must draw again;
  * 4096 random paths of at most 6 segments in the plain room and in scenarios
    F (absorption into expf's denormal and zero range), G (ior 0.6) and H2 (a
    medium inside a heavy BLAS).

Every condition (retry counts, census, finite energies, segment bounds) is
asserted from the oracle before a GPU result is looked at.  A mismatch names
the first differing path, its segment count and its inputs.
"""
import numpy as np
import pytest

import surf_amd
from test_custom_scenes_host import case
from test_oracle_scene_edits import SCENARIOS, PatchedScene
from test_planted_paths_host import RANDOM_SCENES, RANDOM_SEGMENTS, SURFACES, random_paths, retry_paths, scene_of, traced

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
MODES = {"lanes": 0, "wave": 1}


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


@pytest.fixture(scope="module")
def contexts(product_scene):
    """name -> (oracle scene, renderer on the same scene), built on first use."""
    made = {}

    def get(name):
        if name not in made:
            o = scene_of(name)
            p = product_scene if name == "plain" else PatchedScene(product_scene, SCENARIOS[name])
            made[name] = (o, surf_amd.Renderer(p, 8, 8, camera=o.camera_ubo(8, 8)), p)
        return made[name][:2]
    yield get
    for o, r, _ in made.values():
        r.close()
        o.close()


def assert_paths_equal(got, want, inputs, what):
    (ge, gs, gd), (we, ws, wd), (o, d, seeds) = got, want, inputs
    bad = (ge.view(np.uint32) != we.view(np.uint32)).any(axis=1) | (gs != ws) | (gd != wd)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} paths differ; first path {k}: origin {o[k].tolist()} direction "
                             f"{d[k].tolist()} seed 0x{int(seeds[k]):08x}: segments {int(gs[k])} vs the oracle's {int(ws[k])}, "
                             f"energy {ge[k].tolist()} vs {we[k].tolist()}, final seed 0x{int(gd[k]):08x} vs 0x{int(wd[k]):08x}")


@pytest.fixture(scope="module")
def retry_reference(oracle_scene):
    """(surface, max_segments) -> (inputs, the oracle's paths), conditions asserted."""
    done = {}

    def get(surface, max_segments):
        key = (surface, max_segments)
        if key not in done:
            o, d, seeds = retry_paths(SURFACES[surface])
            e, seg, end, census = traced(oracle_scene, o, d, seeds, max_segments)
            assert census["cosine_retries"] >= 120, (surface, census)
            assert np.isfinite(e).all() and (seg <= max_segments).all()
            done[key] = ((o, d, seeds), (e, seg, end))
        return done[key]
    return get


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("max_segments", [1, 8])
@pytest.mark.parametrize("surface", list(SURFACES))
def test_cosine_retry_paths_equal_the_oracle(contexts, retry_reference, surface, max_segments, mode):
    inputs, want = retry_reference(surface, max_segments)
    r = contexts("plain")[1]
    got = r.debug_trace_paths(*inputs, max_segments, MODES[mode])
    assert_paths_equal(got, want, inputs, f"retry seeds toward the {surface}, {max_segments} segments, {mode}")


@pytest.fixture(scope="module")
def random_reference(contexts):
    done = {}

    def get(name):
        if name not in done:
            inputs = random_paths()
            e, seg, end, census = traced(contexts(name)[0], *inputs, RANDOM_SEGMENTS)
            assert np.isfinite(e).all() and (seg >= 1).all() and (seg <= RANDOM_SEGMENTS).all()
            assert census["diffuse"] >= 4096 and census["refract"] >= 20, census
            if name == "F":
                assert census["exp_below_60"] >= 20 and census["exp_zero"] >= 10, census
            if name == "G":
                assert census["tir_outside"] >= 10, census
            if name == "H2":
                assert census["medium_segments"] >= 100 and census["tir_inside"] >= 20, census
            done[name] = (inputs, (e, seg, end))
        return done[name]
    return get


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", RANDOM_SCENES)
def test_random_paths_equal_the_oracle(contexts, random_reference, name, mode):
    inputs, want = random_reference(name)
    r = contexts(name)[1]
    got = r.debug_trace_paths(*inputs, RANDOM_SEGMENTS, MODES[mode])
    assert_paths_equal(got, want, inputs, f"random paths, scene {name}, {mode}")


def test_cutoff_follows_the_context(contexts, oracle_scene):
    """With surf_set_zero_cutoff off the planted paths follow the reference's
    semantics: the oracle's without its cutoff.  Scenario F's paths are the
    ones a cutoff ends (throughput below FLT_MIN after the lens)."""
    inputs = random_paths()
    o, r = contexts("F")
    e, seg, end = o.trace_paths(*inputs, RANDOM_SEGMENTS)
    on = traced(o, *inputs, RANDOM_SEGMENTS)
    assert on[3]["cutoff_kills"] >= 5 and not np.array_equal(on[1], seg), on[3]
    r.set_zero_cutoff(False)
    try:
        got = r.debug_trace_paths(*inputs, RANDOM_SEGMENTS, 0)
    finally:
        r.set_zero_cutoff(None)
    assert_paths_equal(got, (e, seg, end), inputs, "random paths, scene F, cutoff off")


def test_refusals(contexts):
    o, d, seeds = retry_paths(SURFACES["floor"])
    r = contexts("plain")[1]
    for bad in (0, 4097):
        for mode in (0, 1):
            with pytest.raises(surf_amd.SurfError) as err:
                r.debug_trace_paths(o, d, seeds, bad, mode)
            assert err.value.code == -1
    with pytest.raises(surf_amd.SurfError) as err:
        r.debug_trace_paths(o, d, seeds, 4, 2)
    assert err.value.code == -1
    e, seg, end = r.debug_trace_paths(o[:0], d[:0], seeds[:0], 4, 0)
    assert len(e) == len(seg) == len(end) == 0
    # the context still works after the refusals
    e, seg, end = r.debug_trace_paths(o[:3], d[:3], seeds[:3], 4096, 1)
    assert (seg >= 1).all() and np.isfinite(e).all()


def test_wave_mode_is_refused_where_the_wave_walk_is():
    """Ddeep of tests/test_custom_scenes_host.py: a BVH stack of 102 entries, past
    the wave walk's 64.  Mode 1 is refused as surf_set_trace_mode(1) is; mode 0
    answers, and equals the oracle on the scene's own rays."""
    c = case("Ddeep")
    ro, rd = c.all_rays()
    keep = np.isfinite(ro).all(axis=1) & np.isfinite(rd).all(axis=1)
    ro, rd = np.ascontiguousarray(ro[keep][:256]), np.ascontiguousarray(rd[keep][:256])
    seeds = np.arange(1, len(ro) + 1, dtype=np.uint32) * np.uint32(2654435761)
    want = traced(c.oracle, ro, rd, seeds, 4)
    assert np.isfinite(want[0]).all() and (want[1] > 1).sum() >= 16, np.bincount(want[1])
    r = surf_amd.Renderer(c.product(), 8, 8)
    try:
        with pytest.raises(surf_amd.SurfError) as err:
            r.set_trace_mode(1)
        assert err.value.code == -1
        with pytest.raises(surf_amd.SurfError) as err:
            r.debug_trace_paths(ro, rd, seeds, 4, 1)
        assert err.value.code == -1
        assert_paths_equal(r.debug_trace_paths(ro, rd, seeds, 4, 0), want[:3], (ro, rd, seeds), "Ddeep, lanes")
    finally:
        r.close()
