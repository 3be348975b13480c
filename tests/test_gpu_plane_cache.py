"""The cached planes of the per-pixel passes -- first-hit, chain and sampled
feature buffers, ambient occlusion -- follow the camera, the instances and the
scene: one function drops them all (dropDerivedPlanes), and each pass keeps its
planes per key.

Bar: np.array_equal against a fresh Renderer brought to the same state without
ever having read a plane.  What the planes hold is pinned elsewhere
(test_gpu_aov*.py, test_gpu_ao.py compare them to the oracle word for word);
here only the cache is under test, and each case also asserts that the event
changed at least one plane, so a cache that never drops cannot pass.

Frames are test_gpu_aov's 100 x 37.
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from test_gpu_aov import W, H

pytestmark = pytest.mark.gpu

PASSES = {
    "first_hit": lambda r: r.aov(),
    "chain_2_links": lambda r: r.aov_chain(2),
    "sampled_4": lambda r: r.aov_sampled(samples=4),
    "ao_4_first_hit": lambda r: r.ao(samples=4),
    "ao_4_chain": lambda r: r.ao(samples=4, source="chain", max_links=2),
}
EVENTS = ("set_camera", "update_instances", "upload_scene")


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


@pytest.fixture(scope="module")
def updated_scene():
    """The bundled scene half a second on: what update_instances and the re-upload hand over."""
    p = surf_amd.Scene.indoor()
    p.update(0.5)
    yield p
    p.close()


@pytest.fixture(scope="module")
def moved_camera(product_scene):
    ubo = np.frombuffer(product_scene.camera(W, H), np.float32).copy()
    shift = np.array([0.0, 6.0, -12.0], np.float32)      # test_gpu_aov's: a third to most of the pixels miss
    ubo[0:3] = ubo[0:3] + shift                          # position
    ubo[16:19] = ubo[16:19] + shift                      # first_pixel
    return ubo.tobytes()


def cause(event, r, updated_scene, moved_camera):
    if event == "set_camera":
        r.set_camera(moved_camera)
    elif event == "update_instances":
        r.update_instances(updated_scene)
    else:
        d = updated_scene.desc()
        assert surf_amd.load().surf_upload_scene(r.handle, C.byref(d)) == 0


@pytest.fixture(scope="module")
def fresh(product_scene, updated_scene, moved_camera):
    """Every pass's planes from a context that reached the event's state with nothing cached: one context per event."""
    out = {}
    for event in EVENTS:
        if event == "upload_scene":
            r = surf_amd.Renderer(updated_scene, W, H, camera=product_scene.camera(W, H))
        else:
            r = surf_amd.Renderer(product_scene, W, H)
            cause(event, r, updated_scene, moved_camera)
        try:
            out[event] = {name: read(r) for name, read in PASSES.items()}
        finally:
            r.close()
    return out


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("event", EVENTS)
@pytest.mark.parametrize("name", PASSES)
def test_planes_follow_the_event(name, event, product_scene, updated_scene, moved_camera, fresh):
    read = PASSES[name]
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        before = read(r)
        assert same(read(r), before), "a second read of the cached planes"
        cause(event, r, updated_scene, moved_camera)
        after = read(r)
    finally:
        r.close()
    for k in after:
        assert np.array_equal(after[k], fresh[event][name][k]), f"{name} after {event}: plane {k} is not a fresh context's"
    assert not same(after, before), f"{event} changed no plane of {name}: the case proves nothing"


def test_chain_links_and_occlusion_from_the_chain_take_turns(product_scene):
    """The chain planes are kept per max_links and the occlusion pass computes its
    source through the same cache: 2 links, 8, 2 again, with occlusion reads from
    the chain source in between, each against a context that read nothing else."""
    steps = [("chain", 2), ("ao", 2), ("chain", 8), ("ao", 2), ("ao", 8), ("chain", 2)]

    def read(r, what, links):
        return r.aov_chain(links) if what == "chain" else r.ao(samples=4, source="chain", max_links=links)

    want = {}
    for step in dict.fromkeys(steps):
        f = surf_amd.Renderer(product_scene, W, H)
        try:
            want[step] = read(f, *step)
        finally:
            f.close()
    assert not same(want[("chain", 2)], want[("chain", 8)]), "2 and 8 links give the same planes: the test proves nothing"
    assert not same(want[("ao", 2)], want[("ao", 8)])
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        for i, step in enumerate(steps):
            got = read(r, *step)
            for k in got:
                assert np.array_equal(got[k], want[step][k]), f"step {i} {step}: plane {k}"
    finally:
        r.close()
