"""Planted paths on the CPU: the inputs tests/test_gpu_planted_paths.py gives the
GPU, and what they stand on.

A planted path enters Renderer::trace at a caller's origin, direction and RNG
state (OracleScene.trace_paths on the oracle, Renderer.debug_trace_paths on
the device) instead of a camera sample's.  That reaches what no render does:

  * the retry of randomOnHemisphereCosineWeighted (surf_math.cpp:116-134).  It
    needs dot(out, n) == 0, which needs r0 == 1.0f: a 2^-25 event per diffuse
    bounce that no render of the suite has ever drawn.  xorshift32 is
    invertible, so a seed whose SECOND draw (the first is trace's branch draw)
    is one of the 128 states 0xFFFFFF80 .. 0xFFFFFFFF -- all of which rndF
    rounds to 1.0f -- can be planted: seed = inv(inv(s2)).  From (0.5, 2, 0.3)
    toward -y, +x, +z and +y the first hit is the floor, a side wall, the back
    wall and the ceiling, all axis-aligned, where r0 == 1 gives a sample in
    the surface's plane and the loop draws again;
  * shading from anywhere in the room in any direction, not only along what
    the camera sees: 4096 random paths of at most 6 segments, in the plain room
    and in scenarios F, G and H2 of tests/test_oracle_scene_edits.py.

Pinned here, without a GPU: the inverse, the retry counts from the oracle's
census (at least 120 of 128 per surface; the rest take the floor material's
1 % mirror branch), the draw count of a retried bounce, that trace_paths is
the trace() a render runs (a pixel's path planted from its recorded primary
ray and rebuilt RNG state gives the pixel's radiance), and the two debug entry
points' declarations and argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import surf_amd
from test_oracle_scene_edits import SCENARIOS, edited_oracle

F = np.float32
M32 = 0xFFFFFFFF
HEADER = os.path.join(surf_amd.REPO_ROOT, "include", "surf_hip.h")
SURF_ERR_INVALID = -1

START = (0.5, 2.0, 0.3)
SURFACES = {"floor": (0.0, -1.0, 0.0), "side wall": (1.0, 0.0, 0.0), "back wall": (0.0, 0.0, 1.0), "ceiling": (0.0, 1.0, 0.0)}
RANDOM_SCENES = ("plain", "F", "G", "H2")
RANDOM_PATHS, RANDOM_SEGMENTS = 4096, 6


def xorshift(s):
    """RandomU32 (surf_math.cpp:57-63)."""
    s ^= (s << 13) & M32
    s ^= s >> 17
    s ^= (s << 5) & M32
    return s


def xorshift_inverse(s):
    s ^= (s << 5) & M32
    s ^= (s << 10) & M32
    s ^= (s << 20) & M32        # s ^= s << 5 undone
    s ^= s >> 17                # s ^= s >> 17 is its own inverse (34 > 32)
    s ^= (s << 13) & M32
    s ^= (s << 26) & M32        # s ^= s << 13 undone
    return s


def advance(s, draws):
    for _ in range(draws):
        s = xorshift(s)
    return s


def retry_seeds():
    """The 128 seeds whose second draw is 0xFFFFFF80 + k: r0 == 1.0f."""
    return np.array([xorshift_inverse(xorshift_inverse(0xFFFFFF80 + k)) for k in range(128)], np.uint32)


def retry_paths(direction):
    seeds = retry_seeds()
    o = np.tile(np.asarray(START, np.float32), (len(seeds), 1))
    d = np.tile(np.asarray(direction, np.float32), (len(seeds), 1))
    return o, d, seeds


def random_paths(n=RANDOM_PATHS, seed=20240607):
    """Origins uniform in the room (x, z in (-10, 10), y in (-1, 9)), normalised
    normal directions, nonzero seeds."""
    rng = np.random.default_rng(seed)
    o = (rng.random((n, 3), dtype=np.float32) * F(0.98) + F(0.01)) * np.array([20, 10, 20], np.float32) + np.array([-10, -1, -10], np.float32)
    d = rng.standard_normal((n, 3), dtype=np.float32)
    d = (d / np.linalg.norm(d.astype(np.float64), axis=1)[:, None]).astype(np.float32)
    seeds = rng.integers(1, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d), seeds


def scene_of(name):
    return oracle.OracleScene() if name == "plain" else edited_oracle(SCENARIOS[name])


def traced(o_scene, o, d, seeds, max_segments):
    """trace_paths with the cutoff on (what the device runs for a planted path
    by default) and the census of the call: (energy, segments, seeds, census)."""
    oracle.set_zero_cutoff(True)
    try:
        oracle.shade_census()
        e, seg, end = o_scene.trace_paths(o, d, seeds, max_segments)
        census = oracle.shade_census()
    finally:
        oracle.set_zero_cutoff(False)
    return e, seg, end, census


# ---- the inverse -----------------------------------------------------------------

def test_xorshift_inverse_and_the_planted_draw():
    rng = np.random.default_rng(1)
    for s in [1, M32, 0x80000000, 0xFFFFFF80] + rng.integers(1, 1 << 32, 200).tolist():
        assert xorshift_inverse(xorshift(s)) == s and xorshift(xorshift_inverse(s)) == s
        assert oracle.random_u32_stream(s, 1) == [xorshift(s)]
    seeds = retry_seeds()
    assert len(np.unique(seeds)) == 128 and (seeds != 0).all()
    for k, s in enumerate(seeds.tolist()):
        first, second = oracle.random_u32_stream(s, 2)
        assert second == 0xFFFFFF80 + k
        # RandomF32 (surf_math.cpp:70-73): the second draw is r0 == 1.0f
        assert F(second) * F(2.3283064365387e-10) == F(1.0)
    # the state below the range does not round to 1
    assert F(0xFFFFFF7F) * F(2.3283064365387e-10) < F(1.0)


# ---- the retry ---------------------------------------------------------------------

@pytest.mark.parametrize("max_segments", [1, 8])
@pytest.mark.parametrize("surface", list(SURFACES))
def test_planted_seeds_take_the_cosine_retry(oracle_scene, surface, max_segments):
    o, d, seeds = retry_paths(SURFACES[surface])
    t, _, _, inst, _ = oracle_scene.trace_closest(o[:1], d[:1])
    assert inst[0] == {"floor": 0, "side wall": 7, "back wall": 10, "ceiling": 8}[surface] and t[0] > 1.0
    e, seg, end, census = traced(oracle_scene, o, d, seeds, max_segments)
    assert census["cosine_retries"] >= 120, (surface, census)
    assert census["cosine_retries"] <= 128            # one per planted bounce; a later bounce's r0 == 1 is a 2^-25 event
    assert np.isfinite(e).all() and (seg >= 1).all() and (seg <= max_segments).all()
    if max_segments == 1:
        # a retried diffuse bounce draws 10 times (branch, 2 + 2 for the sample, 4 for the light, roulette);
        # the floor material's 1 % mirror branch draws once
        draws = np.array([10 if end[k] == advance(int(s), 10) else 1 if end[k] == advance(int(s), 1) else -1 for k, s in enumerate(seeds)])
        assert (draws > 0).all(), np.flatnonzero(draws < 0)
        assert (draws == 10).sum() == census["cosine_retries"] == census["diffuse"]
        assert (draws == 1).sum() == census["mirror"]
        assert census["mirror"] == 0 if surface == "side wall" else census["mirror"] <= 8
    again = traced(oracle_scene, o, d, seeds, max_segments)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((e, seg, end), again[:3]))


# ---- trace_paths is the trace() a render runs ----------------------------------------

def test_a_planted_pixel_path_gives_the_pixels_radiance(oracle_scene):
    """Pixel p of frame 0: seed initSeed(p), two jitter draws (y first), the lens
    disk's rejection loop (camera.h:59-87), then trace().  The state after those
    draws is rebuilt in numpy; the primary ray is the recorded one."""
    W, H = 32, 24
    acc, _, _ = oracle_scene.render(W, H, 1)
    checked = 0
    for p in range(5, W * H, 37):
        draws = oracle.random_u32_stream(oracle.init_seed(p), 40)
        r = [F(u) * F(2.3283064365387e-10) for u in draws]
        k = 2
        while True:
            sy, sx = r[k] * F(2.0) + F(-1.0), r[k + 1] * F(2.0) + F(-1.0)
            k += 2
            if not sx * sx + sy * sy > F(1.0):
                break
        (eo, ed), _ = oracle_scene.record_rays(W, H, 0, p, p + 1)
        e, seg, _ = oracle_scene.trace_paths(eo[:1], ed[:1], [draws[k - 1]])
        assert seg[0] == len(eo)
        assert np.array_equal(e[0].view(np.uint32), acc[p // W, p % W, :3].view(np.uint32)), (p, e[0], acc[p // W, p % W])
        checked += 1
    assert checked >= 20


# ---- the random paths ------------------------------------------------------------------

@pytest.mark.parametrize("name", RANDOM_SCENES)
def test_random_paths_reach_their_branches(name):
    o, d, seeds = random_paths()
    assert o.dtype == d.dtype == np.float32 and np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (np.abs(o[:, [0, 2]]) < 10).all() and (o[:, 1] > -1).all() and (o[:, 1] < 9).all()
    s = scene_of(name)
    try:
        e, seg, end, census = traced(s, o, d, seeds, RANDOM_SEGMENTS)
    finally:
        s.close()
    assert np.isfinite(e).all() and (seg >= 1).all() and (seg <= RANDOM_SEGMENTS).all()
    assert (seg == RANDOM_SEGMENTS).sum() >= 200 and (seg == 1).sum() >= 20, np.bincount(seg)
    assert census["diffuse"] >= 4096 and census["mirror"] >= 50 and census["refract"] >= 20, census
    if name == "F":
        assert census["exp_below_60"] >= 20 and census["exp_zero"] >= 10, census
    if name == "G":
        assert census["tir_outside"] >= 10, census
    if name == "H2":
        assert census["medium_segments"] >= 100 and census["tir_inside"] >= 20, census


# ---- the two entry points' declarations and argument checks ------------------------------

PROTOTYPES = {
    "surf_debug_math": r"surf_ctx\s*\*\s*\w*,\s*int\s+\w+,\s*uint32_t\s+\w+,\s*const\s+float\s*\*\s*\w*,\s*float\s*\*\s*\w*",
    "surf_debug_math_host": r"int\s+\w+,\s*uint32_t\s+\w+,\s*const\s+float\s*\*\s*\w*,\s*float\s*\*\s*\w*",
    "surf_debug_trace_paths": (r"surf_ctx\s*\*\s*\w*,\s*uint32_t\s+\w+,\s*const\s+float\s*\*\s*\w*,\s*const\s+float\s*\*\s*\w*,"
                               r"\s*const\s+uint32_t\s*\*\s*\w*,\s*uint32_t\s+\w+,\s*int\s+\w+,\s*float\s*\*\s*\w*,\s*uint32_t\s*\*\s*\w*"),
}


def test_entry_points_declared_and_exported_at_abi_4():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = surf_amd.load()
    for name, args in PROTOTYPES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), code), f"{name} is not declared with its prototype"
        assert hasattr(lib, name), f"{name} is not exported"
    for k, name in enumerate(n.upper() for n in surf_amd.MATH_OPS):
        assert re.search(r"\bSURF_MATH_%s\s*=\s*%d\b" % (name, k), code), name
    assert lib.surf_abi_version() == 4


def test_null_and_range_arguments_are_invalid_not_fatal():
    lib = surf_amd.load()
    x = np.zeros(4, np.float32)
    y = np.zeros(8, np.float32)
    od = np.zeros(6, np.float32)
    s = np.ones(2, np.uint32)
    p = lambda a: a.ctypes.data
    assert lib.surf_debug_math(None, 0, 4, p(x), p(y)) == SURF_ERR_INVALID
    assert lib.surf_debug_trace_paths(None, 2, p(od), p(od), p(s), 4, 0, p(y), p(s)) == SURF_ERR_INVALID
    h = C.c_void_p()
    if lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0:      # a context needs a device; the NULL-context calls above do not
        try:
            assert lib.surf_debug_math(h, 4, 4, p(x), p(y)) == SURF_ERR_INVALID
            assert lib.surf_debug_math(h, -1, 4, p(x), p(y)) == SURF_ERR_INVALID
            assert lib.surf_debug_math(h, 0, 4, None, p(y)) == SURF_ERR_INVALID
            assert lib.surf_debug_math(h, 0, 4, p(x), None) == SURF_ERR_INVALID
            assert lib.surf_debug_trace_paths(h, 2, None, p(od), p(s), 4, 0, p(y), p(s)) == SURF_ERR_INVALID
            for bad in (0, 4097):
                assert lib.surf_debug_trace_paths(h, 2, p(od), p(od), p(s), bad, 0, p(y), p(s)) == SURF_ERR_INVALID
            assert lib.surf_debug_trace_paths(h, 2, p(od), p(od), p(s), 4, 2, p(y), p(s)) == SURF_ERR_INVALID
        finally:
            lib.surf_destroy(h)


def test_python_wrappers_check_before_the_library():
    r = surf_amd.Renderer.__new__(surf_amd.Renderer)     # no context: the checks come before any use of one
    r._h = None
    with pytest.raises(ValueError):
        r.debug_math("tanf", np.zeros(3, np.float32))
    with pytest.raises(ValueError):
        r.debug_trace_paths(np.zeros((2, 3)), np.zeros((3, 3)), np.ones(2), 4)
