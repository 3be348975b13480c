"""GPU parity outside the one picture the other render tests share: the scenarios
of tests/test_oracle_scene_edits.py (a camera outside the room, a pinhole,
solid and black skies, a clear pane in place of the green wall, a lens that
both reflects and refracts, no lights at all, an emissive Suzanne) rendered by
the HIP wavefront path and by the oracle with the same edits.

They reach what a closed room seen from main.cpp's camera never does, or does
for one sample in 600 that slips out between two walls and sees the gradient:
shadePath's miss branch (background types 0, 1 and other; a miss with the
medium flag set; frame completion and the next sample of a chain after a path
that ends on its first segment; the radiance add of k_shade and of both drain
engines), cameraSample without a lens, a moved camera in k_regen, chainNext
and classifyPixels, the mirror / dielectric / diffuse choice inside a medium,
S.nLights == 0, and sampleNEE / k_connect with an emitter whose BLAS is large.

Scenarios F to J keep the view and push the materials to their extremes
(absorption into expf's denormal and zero range, an ior of 0.6 and of 3,
refl + refr > 1 and refl == 1, a medium inside a heavy BLAS, albedo above 1,
at 0 and below 0, a denormal emitter strength, a non-emitter with emit > 0):
the branches of shadePath that one material table never takes.  Their
conditions are floors on the oracle's shading census (CENSUS_FLOORS).

Bar: bit-exact accumulator words and equal event counts, as
tests/test_gpu_parity.py.  Each render's conditions (enough misses, shadow
rays where they are expected, no path past 4096 segments) are asserted from
the oracle's counters before the GPU result is looked at.

The product side of a scenario is PatchedScene: the product's own buffers with
the edited records; test_patched_buffers_equal_the_edited_export pins it to
the oracle's export on the CPU.  The camera UBO is the oracle's.
"""
import numpy as np
import pytest

import oracle
import surf_amd
from test_gpu_aov import W as AW, H as AH, assert_planes_equal, camera_rays, expected_planes
from test_gpu_aov_chain import chain_planes
from test_gpu_parity import _assert_bitexact, _assert_counts
from test_oracle_scene_edits import SCENARIOS, PatchedScene, check_conditions, edited_oracle, render_counted

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(900)]
W, H, FRAMES = 64, 48, 3
HEAVY = (3, 4, 5)            # the three largest BLASes' instances: both Suzannes and the lens (setKeys)


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


@pytest.fixture(scope="module")
def scenes(product_scene):
    """name -> (edited oracle scene, patched product scene), built on first use."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = (edited_oracle(SCENARIOS[name]), PatchedScene(product_scene, SCENARIOS[name]))
        return made[name]
    yield get
    for o, _ in made.values():
        o.close()


@pytest.fixture(scope="module")
def reference(scenes):
    """(name, W, H, frames) -> (radiance, counters) of the oracle, once per module,
    with _render_both's cutoff handling: the radiance in reference semantics
    (no cutoff), the event counts with the cutoff the GPU runs by default, and
    the two radiances equal bit for bit.  The scenario's conditions are
    asserted here, so no GPU render starts on an input that misses them."""
    done = {}

    def get(name, w, h, frames):
        key = (name, w, h, frames)
        if key not in done:
            o = scenes(name)[0]
            c2, cnt = render_counted(o, w, h, frames)
            miss = check_conditions(name, o, cnt, c2)
            c, _, _ = o.render(w, h, frames)
            assert np.array_equal(c.view(np.uint32), c2.view(np.uint32)), "cutoff changed the oracle's radiance"
            c.setflags(write=False)
            print(f"scenario {name} {w}x{h}x{frames}: samples {cnt['samples']} misses {cnt['n_ext'] - cnt['n_hit']} "
                  f"({miss:.3f} per sample) shadow rays {cnt['n_shadow']} unoccluded {cnt['n_unocc']} "
                  f"longest path {cnt['max_segments']} lights {o.light_count()}")
            done[key] = (c, cnt)
        return done[key]
    return get


def renderer(scenes, name, w, h, **kw):
    o, p = scenes(name)
    return surf_amd.Renderer(p, w, h, camera=o.camera_ubo(w, h), **kw)


# ---- 1. every scenario through the wavefront and both drain engines ------------

@pytest.mark.parametrize("policy,coop,engine", [((1, 0, 0), 0, "lanes"), ((1 << 30, 0, 8), 1 << 30, "pair"),
                                                ((1 << 30, 0, 8), 1 << 30, "coop")],
                         ids=["wavefront-to-end", "pair-from-start", "coop-from-start"])
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_scenario_bitexact(scenes, reference, name, policy, coop, engine, monkeypatch):
    """64 x 48, 3 frames of each scenario: k_shade to the end, and the partner-wave
    and the one-path-per-wave drain (shadePath<true>) as soon as the stream has
    nothing left to issue.  The drains take what is in flight at a replay
    boundary, and outside the room no path lives through a whole replay of 16
    phases: a pool of 64 paths keeps the issue going until the last phases, so
    that some paths are still in flight when it ends (2 in A, 12 in B, 25 in C
    as measured; test_scenario_spp4_bitexact hands the drains whole frames)."""
    monkeypatch.setenv("SURF_TAIL_PAIR", "0" if engine == "coop" else "1")
    c, cnt = reference(name, W, H, FRAMES)
    r = renderer(scenes, name, W, H, pool_capacity=None if engine == "lanes" else 64)
    try:
        r.set_tail_policy(*policy)
        r.set_tail_coop(coop)
        r.render(FRAMES, 0, 0)
        g = r.accumulator()
        st = r.stats()
    finally:
        r.close()
    print(f"scenario {name} {engine}: drain paths {st['tail_survivors']}, samples ended there {st['tail_paths']}, "
          f"drain rays {st['n_ext'] - st['n_ext_wavefront']} of {st['n_ext']}")
    if engine == "lanes":
        assert st["tail_survivors"] == 0, "the wave engines must stay out of a wavefront-to-the-end run"
    else:
        assert st["tail_survivors"] > 0, f"the {engine} drain did not run"
    assert np.all(g[..., 3] == FRAMES) and st["samples"] == W * H * FRAMES
    _assert_bitexact(g, c, f"scenario {name}, {engine} {policy}")
    _assert_counts(st, cnt)


# ---- 2. multi-sample frames: chainNext after a miss, under a moved camera -------

@pytest.mark.parametrize("engine", ["wavefront", "pair", "coop"])
@pytest.mark.parametrize("name", ["A", "C", "F", "H2", "H3"])
def test_scenario_spp4_bitexact(scenes, name, engine, monkeypatch):
    """2 frames of 4 chained samples (orc_render_spp), the throughput cutoff on on
    both sides (the conditions are stated for it): in A almost every sample ends
    in a miss, many on its first segment, and the next sample of the pixel
    starts from the state it left, drawn through the moved camera -- by k_shade
    with default settings, and inside each drain engine: a window of one frame
    (4 passes) starves the stream while the frame's chains are in flight, so
    the drain takes them and draws their remaining samples itself."""
    K, FR = 4, 2
    o = scenes(name)[0]
    c, cnt = render_counted(o, W, H, FR, spp=K)
    check_conditions(name, o, cnt, c)
    monkeypatch.setenv("SURF_TAIL_PAIR", "0" if engine == "coop" else "1")
    r = renderer(scenes, name, W, H, frame_batch=None if engine == "wavefront" else K)
    try:
        r.set_zero_cutoff(True)
        if engine != "wavefront":
            r.set_tail_policy(1 << 30, 0, 8)
            r.set_tail_coop(1 << 30)
        r.render(FR, 0, 0, spp=K)
        g = r.accumulator()
        st = r.stats()
    finally:
        r.close()
    print(f"scenario {name} spp {K} {engine}: drain paths {st['tail_survivors']}, samples ended there {st['tail_paths']}, "
          f"drain rays {st['n_ext'] - st['n_ext_wavefront']} of {st['n_ext']}")
    if engine != "wavefront":
        assert st["tail_survivors"] >= 100 and st["tail_paths"] >= st["tail_survivors"], (st["tail_survivors"], st["tail_paths"])
    assert np.all(g[..., 3] == FR * K) and st["samples"] == W * H * FR * K
    _assert_bitexact(g, c, f"scenario {name}, {FR} frames x {K} samples, {engine}")
    _assert_counts(st, cnt)


# ---- 3. a multi-frame stream: the issue order under the edited scene and camera -

@pytest.mark.parametrize("name", ["A", "C"])
def test_scenario_issue_order_stream_bitexact(scenes, reference, name):
    """96 x 64, 8 frames as one stream with default settings: the pixel classes of
    the heavy-pixels-first issue order come from the centre rays of the camera
    in use.  From outside (A) the front wall hides every heavy instance, so no
    pixel is heavy and the stream stays frame-major -- the default camera would
    find hundreds; in C the order is engaged as in the closed room."""
    w, h, frames = 96, 64, 8
    c, cnt = reference(name, w, h, frames)
    o = scenes(name)[0]
    first = o.trace_closest(*camera_rays(o.camera_ubo(w, h), w, range(h)))[3]
    heavy_want = int(np.isin(first, HEAVY).sum())
    r = renderer(scenes, name, w, h)
    try:
        r.render(frames, 0, 0)
        heavy, permuted = r.debug_issue_order()
        g = r.accumulator()
        st = r.stats()
    finally:
        r.close()
    if name == "A":
        assert heavy_want == 0 and (heavy, permuted) == (0, 0), (heavy_want, heavy, permuted)
    else:
        assert heavy_want > 100 and permuted == frames, (heavy_want, heavy, permuted)
        # the host's centre rays are not written operation for operation: a silhouette pixel may differ
        assert abs(heavy - heavy_want) <= 4, (heavy, heavy_want)
    _assert_bitexact(g, c, f"scenario {name}, {w}x{h}x{frames} stream")
    _assert_counts(st, cnt)


# ---- 4. an emitter with a large BLAS: the staged / global emitter walk ----------

@pytest.mark.parametrize("staged", ["1", "0"], ids=["light-blas-in-lds-asked", "light-blas-global"])
def test_large_emitter_takes_the_global_walk_bitexact(scenes, reference, staged, monkeypatch):
    """Scenario E.  k_connect stages the emitters' BLAS in LDS only when every
    light instance shares one BLAS whose compact records and triangles fit
    20 KiB (setKeys, compactBlases: scene_upload.hip).  Two cubes and a Suzanne
    share none, and Suzanne's 15,744 triangles would not fit: with the switch on
    or off the launch must take the global walk -- and sampleNEE picks among
    15,744 triangles for a third of its samples."""
    monkeypatch.setenv("SURF_LDS_LIGHTBLAS", staged)
    c, cnt = reference("E", W, H, FRAMES)
    r = renderer(scenes, "E", W, H)
    try:
        r.render(FRAMES, 0, 0)
        g = r.accumulator()
        st = r.stats()
        assert r.debug_connect_staging() == (0, 0), "a Suzanne-sized emitter BLAS must not be staged"
    finally:
        r.close()
    _assert_bitexact(g, c, f"scenario E, light BLAS staging asked={staged}")
    _assert_counts(st, cnt)


# ---- 5. the feature planes of the edited scenes --------------------------------

@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_scenario_feature_planes_bitexact(scenes, name):
    """r.aov() and r.aov_chain(8) against the numpy restatements of
    tests/test_gpu_aov.py and tests/test_gpu_aov_chain.py, fed by the edited
    oracle.  In C the chains that leave through the pane end in the tinted miss
    after at least one link -- the branch the closed room cannot reach."""
    o = scenes(name)[0]
    ubo = o.camera_ubo(AW, AH)
    want, info = expected_planes(o, ubo, AW, range(AH))
    chain, cinfo = chain_planes(o, ubo, AW, range(AH), 8)
    miss = 1.0 - info["hit"].mean()
    tinted = cinfo["ended_miss"] & (cinfo["links"] >= 1)
    if name == "C":
        assert tinted.sum() >= 20, tinted.sum()
        alb = chain["albedo"].reshape(-1, 4)[tinted]
        assert (alb[:, 3] == 0).all() and (alb[:, :3] > 0).all()
        # some of them come through the lens: a tint that is not the pane's 1
        assert (cinfo["links"][tinted] >= 2).any()
    else:
        assert 0.05 <= miss <= 0.8, f"{name}: {miss:.3f} of the pixels miss"
        assert info["gradient"] == (name == "A")
    r = renderer(scenes, name, AW, AH)
    try:
        assert_planes_equal(r.aov(), want, f"scenario {name} first hit")
        assert_planes_equal(r.aov_chain(8), chain, f"scenario {name} chain")
    finally:
        r.close()


# Pixels (of 3,700) whose chain takes the link at least once, as the numpy restatement
# counts them: (observed, floor asserted -- about half).
EXTREME_LINKS = {
    "G": {"tir_outside": (32, 16), "refract": (5, 2)},                       # ior 0.6: reflection on entry
    "H": {"reflect": (836, 400), "refract": (40, 20)},                       # refl 1, and refl + refr > 1 either way round
    "H3": {"tir_outside": (24, 12), "tir": (49, 24), "refract": (71, 35)},   # ior 0.7 through a heavy BLAS, absorbing
}


@pytest.mark.parametrize("name", list(EXTREME_LINKS))
def test_extreme_material_feature_planes_bitexact(scenes, name):
    """r.aov() and r.aov_chain(16) of G, H and H3.  The chain's delta rule
    (include/surf_hip.h: a link where refl + refr >= 0.5, a dielectric one where
    refl < refr, refraction where cos2 > 0 whichever side the ray is on) is the
    numpy restatement's as it stood: total internal reflection on entry (an ior
    below 1) is its `dielectric & ~refract` with the medium flag clear, counted
    as tir_outside.  No bundled material reaches that, nor a mirror of
    reflectivity 1, nor a dielectric whose refl + refr passes 1."""
    o = scenes(name)[0]
    ubo = o.camera_ubo(AW, AH)
    want, _ = expected_planes(o, ubo, AW, range(AH))
    chain, cinfo = chain_planes(o, ubo, AW, range(AH), 16)
    for key, (_, floor) in EXTREME_LINKS[name].items():
        took = int((cinfo[key] > 0).sum())
        assert took >= floor, f"{name}: {took} pixels take a {key} link"
    assert np.isfinite(chain["albedo"]).all() and np.isfinite(chain["position"][..., :3]).all()
    r = renderer(scenes, name, AW, AH)
    try:
        assert_planes_equal(r.aov(), want, f"scenario {name} first hit")
        assert_planes_equal(r.aov_chain(16), chain, f"scenario {name} chain")
    finally:
        r.close()


# ---- 6. set_camera back to the default drops the stream and the plane caches ----

def test_camera_back_to_default_drops_every_cache(scenes, reference, oracle_scene):
    """Scenario A edits nothing but the view.  After its render and plane reads,
    set_camera(the default UBO) on the same context must give the plain
    scene's render and planes: the sample stream, the captured graph, the pixel
    classes and both plane caches follow the camera."""
    c_a, cnt_a = reference("A", W, H, FRAMES)
    ubo = oracle_scene.camera_ubo(W, H)
    oracle.set_zero_cutoff(True)
    try:
        c, cnt, _ = oracle_scene.render(W, H, FRAMES)
    finally:
        oracle.set_zero_cutoff(False)
    want, _ = expected_planes(oracle_scene, ubo, W, range(H))
    chain, _ = chain_planes(oracle_scene, ubo, W, range(H), 8)
    r = renderer(scenes, "A", W, H)
    try:
        r.render(FRAMES, 0, 0)
        _assert_bitexact(r.accumulator(), c_a, "scenario A before the camera moves back")
        moved = r.aov()
        r.aov_chain(8)
        r.set_camera(ubo)
        r.clear_accumulator()
        r.render(FRAMES, 0, 0)
        g = r.accumulator()
        st = r.stats()
        _assert_bitexact(g, c, "default camera after scenario A")
        _assert_counts(st, cnt)
        back = r.aov()
        assert_planes_equal(back, want, "first-hit planes after the camera moved back")
        assert_planes_equal(r.aov_chain(8), chain, "chain planes after the camera moved back")
        assert not np.array_equal(back["id"], moved["id"])
    finally:
        r.close()
