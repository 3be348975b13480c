"""The surfel sensor on the CPU: its declarations, its refusals, and the numpy
restatement tests/test_gpu_surfel_sensor.py holds the device to.

surf_set_surfel_sensor (include/surf_hip.h) starts every sample of surf_render
at a caller's surface point instead of at the camera.  Restated here from the
header's definition with what the suite already has: init_seed, cosine_sample
and pixel_index of tests/test_gpu_ao.py (the path tracer's own seed and
cosine-weighted direction, retry included), and the oracle's planted paths
(OracleScene.trace_paths through traced() of tests/test_planted_paths_host.py,
cutoff on, as the device runs one-sample frames):

    valid(lp)  = N.x != 0 || N.y != 0 || N.z != 0
    seed       = initSeed(p + 1799 * (first + k * spp))        sample 0 of frame k
               = the state the previous sample's path left      sample j > 0
    R          = cosineSample(seed, N);  o = P + 1e-5f * R;  d = R
    energy     = trace(o, d, seed)                              the oracle's, as planted
    A[lp]     += (energy, 1)                                    per sample, in order

Pinned here, without a GPU: the three entry points and the ABI version, the
NULL refusals, the Python wrappers' shape and dtype checks, and that the
restatement reaches its branches on the two inputs the GPU tests start from (a
32 x 24 grid of floor texels and the 32 x 24 view's first-hit planes)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import surf_amd
from test_gpu_ao import cosine_sample, init_seed, pixel_index
from test_gpu_aov import expected_planes
from test_planted_paths_host import traced

F = np.float32
U = np.uint32
HEADER = os.path.join(surf_amd.REPO_ROOT, "include", "surf_hip.h")
SURF_ERR_INVALID = -1
GW, GH = 32, 24
FLOOR = (-9.0, -9.0, 9.0, 9.0, -1.0)        # x0, z0, x1, z1, y: inside the floor's 20 x 20 at y = -1
EMITTERS = (1, 2)                           # the bundled scene's two light cubes (instance ids)
CAP = 12                                    # max_segments of every spp > 1 case


# ---- the restatement -------------------------------------------------------------------------------

def floor_grid(w, h, x0, z0, x1, z1, y):
    """(position, normal), (h, w, 4) float32 each: upward-facing texels at the cell centres of the
    rectangle, every step in f32 (examples/render_baked.cpp computes the same)."""
    tx, ty = np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32)
    px = F(x0) + ((tx + F(0.5)) / F(w)) * (F(x1) - F(x0))
    pz = F(z0) + ((ty + F(0.5)) / F(h)) * (F(z1) - F(z0))
    pos, nrm = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    pos[..., 0], pos[..., 1], pos[..., 2] = px[None, :], F(y), pz[:, None]
    nrm[..., 1] = F(1.0)
    assert px.dtype == np.float32 and pz.dtype == np.float32
    return pos, nrm


def checker_invalid(nrm, keep=lambda bx, by: not (bx % 2 == 0 and by % 2 == 0)):
    """A copy of the normals with a quarter of the texels invalid: the 2 x 2 blocks at even block coordinates."""
    n = nrm.copy()
    h, w = n.shape[:2]
    for y in range(h):
        for x in range(w):
            if not keep(x // 2, y // 2):
                n[y, x, :3] = 0.0
    return n


def valid_texels(nrm):
    n = np.asarray(nrm, np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return (n[:, 0] != F(0.0)) | (n[:, 1] != F(0.0)) | (n[:, 2] != F(0.0))      # a NaN component: valid


def bake_samples(osc, pos, nrm, width, rows, frames, spp=1, max_segments=0, first=0):
    """The sensor's samples: (valid (npx,) bool, energy[k][j] (n_valid, 3) float32 of sample j of frame k,
    info).  info sums the oracle's census over every call and keeps the segment counts and first rays."""
    assert spp == 1 or max_segments == CAP, "every multi-sample case is capped: no oracle path runs unbounded with the cutoff's seed chain"
    P = np.asarray(pos, np.float32).reshape(-1, 4)[:, :3]
    N = np.asarray(nrm, np.float32).reshape(-1, 4)[:, :3]
    valid = valid_texels(nrm)
    idx = np.flatnonzero(valid)
    p = pixel_index(width, rows)[idx]
    Nv, Pv = np.ascontiguousarray(N[idx]), P[idx]
    energy, census, segs, firsts = [], {}, [], []
    for k in range(frames):
        with np.errstate(over="ignore"):
            seed = init_seed(p + U(1799) * U((first + k * spp) & 0xFFFFFFFF))
        chain = []
        for j in range(spp):
            R = cosine_sample(seed, Nv)                  # advances seed in place
            O = Pv + F(1e-5) * R
            assert O.dtype == np.float32 and R.dtype == np.float32
            e, seg, end, c = traced(osc, O, R, seed, max_segments) if len(idx) else (np.zeros((0, 3), F), np.zeros(0, U), seed, {})
            for name, v in c.items():
                census[name] = census.get(name, 0) + v
            chain.append(e)
            segs.append(seg)
            firsts.append((O, R, e))
            seed = np.array(end, np.uint32)
        energy.append(chain)
    return valid, energy, {"census": census, "segments": segs, "first": firsts, "index": idx}


def bake_add(A, valid, energy_kj, active=None):
    """One sample added to the records of the valid texels (those of `active`, a flat bool mask, if given)."""
    npx = len(valid)
    r = np.zeros((npx, 4), np.float32)
    r[np.flatnonzero(valid), :3] = energy_kj
    r[valid, 3] = F(1.0)
    on = valid if active is None else (valid & np.asarray(active, bool).reshape(-1))
    out = np.where(on[:, None], A.reshape(npx, 4) + r, A.reshape(npx, 4))
    assert out.dtype == np.float32
    return out.reshape(A.shape)


def bake_expected(osc, pos, nrm, width, rows, frames, spp=1, max_segments=0, first=0, active=None):
    """(accumulator (len(rows), width, 4), valid, info) of a bake from an empty accumulator."""
    rows = list(rows)
    valid, energy, info = bake_samples(osc, pos, nrm, width, rows, frames, spp, max_segments, first)
    A = np.zeros((len(rows), width, 4), np.float32)
    for chain in energy:
        for e in chain:
            A = bake_add(A, valid, e, active)
    return A, valid, info


def frame_planes(valid, energy, shape):
    """The per-frame (H, W, 4) radiance planes of an spp-1 bake (w = 1 on valid texels), for the loop restatements."""
    out = []
    for chain in energy:
        r = np.zeros((len(valid), 4), np.float32)
        r[np.flatnonzero(valid), :3] = chain[0]
        r[valid, 3] = F(1.0)
        out.append(r.reshape(shape))
    return out


# ---- declarations ----------------------------------------------------------------------------------

PROTOTYPES = {
    "surf_set_surfel_sensor": r"surf_ctx\s*\*\s*\w*,\s*const\s+float\s*\*\s*\w*,\s*const\s+float\s*\*\s*\w*",
    "surf_set_surfel_sensor_device": r"surf_ctx\s*\*\s*\w*,\s*const\s+void\s*\*\s*\w*,\s*const\s+void\s*\*\s*\w*",
    "surf_get_sensor": r"surf_ctx\s*\*\s*\w*,\s*int\s*\*\s*\w*,\s*uint32_t\s*\*\s*\w*",
}


def test_entry_points_declared_and_exported_at_abi_4():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = surf_amd.load()
    for name, args in PROTOTYPES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), code), f"{name} is not declared with its prototype"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+SURF_ABI_VERSION\s+4\b", code) and lib.surf_abi_version() == 4
    assert (surf_amd.SENSOR_CAMERA, surf_amd.SENSOR_SURFELS) == (0, 1)
    for k, name in enumerate(("CAMERA", "SURFELS")):
        assert re.search(r"#define\s+SURF_SENSOR_%s\s+%d\b" % (name, k), code), name
    # the definition travels with the header: validity (NaN included), the unnormalized N, what the accumulator estimates
    flat = re.sub(r"[\s*]+", " ", text)
    for phrase in ("a NaN normal component makes the texel valid", "the library does not normalize it", "estimates E / pi"):
        assert phrase in flat, phrase


def test_null_arguments_are_invalid_not_fatal():
    lib = surf_amd.load()
    a = np.zeros((8, 8, 4), np.float32)
    k, v = C.c_int(7), C.c_uint32(7)
    p = a.ctypes.data
    assert lib.surf_set_surfel_sensor(None, p, p) == SURF_ERR_INVALID
    assert lib.surf_set_surfel_sensor(None, None, None) == SURF_ERR_INVALID
    assert lib.surf_set_surfel_sensor_device(None, p, p) == SURF_ERR_INVALID
    assert lib.surf_get_sensor(None, C.byref(k), C.byref(v)) == SURF_ERR_INVALID
    assert b"NULL" in lib.surf_last_error(None)
    h = C.c_void_p()
    # A context needs a device, so on a machine without one the rest of this test does not run: the one-NULL refusals on
    # a live context are asserted again, unconditionally, in tests/test_gpu_surfel_sensor.py::test_status_codes.
    if lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0:
        try:
            assert lib.surf_set_surfel_sensor(h, p, None) == SURF_ERR_INVALID
            assert lib.surf_set_surfel_sensor(h, None, p) == SURF_ERR_INVALID
            assert lib.surf_set_surfel_sensor_device(h, p, None) == SURF_ERR_INVALID
            assert lib.surf_get_sensor(h, C.byref(k), C.byref(v)) == 0 and (k.value, v.value) == (0, 64)
            assert lib.surf_get_sensor(h, None, None) == 0
        finally:
            lib.surf_destroy(h)


def test_python_wrappers_check_before_the_library():
    r = surf_amd.Renderer.__new__(surf_amd.Renderer)     # no context: the checks come before any use of one
    r._h = None
    r.width, r.height, r.rows = 8, 6, np.arange(6, dtype=np.uint32)
    good = np.zeros((6, 8, 4), np.float32)
    for pos, nrm in ((good, np.zeros((6, 8, 3), np.float32)), (np.zeros((8, 6, 4), np.float32), good), (good.astype(np.float64), good),
                     (good, good.astype(np.float16)), (good[:5], good), (good, None), (None, good), (np.zeros(6 * 8 * 4 + 1, np.float32), good)):
        with pytest.raises(ValueError):
            r.set_surfel_sensor(pos, nrm)
        with pytest.raises(ValueError):
            r.bake(pos, nrm, 1)
    for ptrs in ((0, 16), (16, 0), (None, 16)):
        with pytest.raises(ValueError):
            r.set_surfel_sensor_device(*ptrs)
    pos, nrm = r._surfel_planes(good.reshape(-1), good)   # flat planes of the right size pass
    assert pos.shape == (6 * 8 * 4,) and nrm.shape == (6, 8, 4)


# ---- the restatement reaches its branches ----------------------------------------------------------

def test_grid_and_validity():
    pos, nrm = floor_grid(GW, GH, *FLOOR)
    assert pos[0, 0, 0] == F(-9.0) + (F(0.5) / F(32)) * F(18.0) and pos[GH - 1, 0, 2] == F(-9.0) + (F(23.5) / F(24)) * F(18.0)
    assert (pos[..., 1] == F(-1.0)).all() and (np.abs(pos[..., [0, 2]]) < 9).all()
    assert valid_texels(nrm).all()
    n = checker_invalid(nrm)
    v = valid_texels(n).reshape(GH, GW)
    assert v.sum() == GW * GH * 3 // 4 and not v[0, 0] and not v[1, 1] and v[0, 2] and v[2, 0] and not v[4, 4]
    odd = np.zeros((1, 4, 4), np.float32)
    odd[0, 0, 2], odd[0, 1, 0], odd[0, 2, 3] = -0.0, np.nan, 1.0          # -0: invalid; NaN: valid; w alone: invalid
    assert valid_texels(odd).tolist() == [False, True, False, False]


def test_restatement_reaches_its_branches(oracle_scene):
    pos, nrm = floor_grid(GW, GH, *FLOOR)
    A, valid, info = bake_expected(oracle_scene, pos, nrm, GW, range(GH), 2)
    assert valid.all() and (A[..., 3] == F(2.0)).all() and np.isfinite(A).all()
    seg = np.concatenate(info["segments"])
    assert (seg >= 3).sum() >= 1, np.bincount(seg)
    # a diffuse bounce with a shadow ray: the census counts the bounces, not their shadow rays (planted paths return no
    # event counts), but with lights in the scene every diffuse bounce samples one; the device's own count of the shadow
    # rays of this bake is asserted in tests/test_gpu_surfel_sensor.py::test_floor_grid_bitexact
    assert info["census"]["diffuse"] >= 1 and oracle_scene.light_count() >= 1
    lit = 0
    for O, R, e in info["first"]:
        _, _, _, inst, _ = oracle_scene.trace_closest(O, R)
        lit += int((np.isin(inst, EMITTERS) & (e.sum(axis=1) > 0)).sum())
    assert lit >= 1, "no first segment meets an emitter with energy: the last-bounce-specular start would not be exercised"
    # (the view) the 32 x 24 first-hit planes, sky pixels invalid, the lens among them
    planes, pinfo = expected_planes(oracle_scene, oracle_scene.camera_ubo(GW, GH), GW, range(GH))
    vvalid = valid_texels(planes["normal"])
    assert np.array_equal(vvalid, pinfo["hit"].reshape(-1))                 # a miss's normal is 0: the planes go in as they are
    Av, v2, vinfo = bake_expected(oracle_scene, planes["position"], planes["normal"], GW, range(GH), 2)
    c = vinfo["census"]
    assert c["dielectric_outside"] + c["refract"] + c["fresnel_reflect"] >= 1, c
    assert (Av.reshape(-1, 4)[~v2] == 0).all() and (Av.reshape(-1, 4)[v2, 3] == F(2.0)).all()
    again = bake_expected(oracle_scene, planes["position"], planes["normal"], GW, range(GH), 2)[0]
    assert np.array_equal(again.view(np.uint32), Av.view(np.uint32))


def test_chained_samples_continue_the_seed(oracle_scene):
    """spp = 2, capped: sample 1 starts from the state sample 0's path left, so it differs from frame 1's first sample."""
    pos, nrm = floor_grid(8, 4, *FLOOR)
    _, e2, _ = bake_samples(oracle_scene, pos, nrm, 8, range(4), 1, spp=2, max_segments=CAP)
    _, e1, _ = bake_samples(oracle_scene, pos, nrm, 8, range(4), 2, spp=1, max_segments=CAP)
    assert np.array_equal(e2[0][0].view(U), e1[0][0].view(U))
    assert not np.array_equal(e2[0][1].view(U), e1[1][0].view(U))
