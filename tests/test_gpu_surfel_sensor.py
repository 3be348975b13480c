"""The surfel sensor on the device against its numpy restatement
(tests/test_surfel_sensor_host.py: the header's definition on the oracle's
planted paths).  Every comparison is bit for bit: there is no tolerance.

The cutoff is on on both sides -- traced() switches the oracle's on, the device
runs one-sample frames with it by default and the multi-sample cases switch it
on -- and every multi-sample case is capped at 12 segments, so no oracle path
runs unbounded through the lens."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import surf_amd
from surf_amd import ShardSpec
from test_adaptive_host import np_add_frame, np_mask
from test_gpu_aov import W, H, expected_planes, read_pfm
from test_robust_host import np_halves
from test_surfel_sensor_host import (CAP, FLOOR, GH, GW, bake_add, bake_expected, bake_samples, checker_invalid, floor_grid, frame_planes,
                                     valid_texels)

pytestmark = pytest.mark.gpu
F = np.float32
SURF_ERR_INVALID, SURF_ERR_NO_SCENE = -1, -4


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def assert_acc_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: {got.shape} vs {want.shape}"
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (f"{what}: {len(bad)} words differ, first (row, x, channel) {bad[:4].tolist()}: "
                           f"got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


class Floor:
    """Case 1's input -- the 32 x 24 floor grid, a quarter of its texels invalid in a checker of 2 x 2 blocks --
    and its restated samples, computed once and shared, read only."""

    def __init__(self, osc):
        self.osc = osc
        self.pos, full = floor_grid(GW, GH, *FLOOR)
        self.nrm = checker_invalid(full)
        self.valid, self.energy, self.info = bake_samples(osc, self.pos, self.nrm, GW, range(GH), 8)
        self.n_valid = int(self.valid.sum())
        for a in (self.pos, self.nrm, self.valid):
            a.setflags(write=False)

    def acc(self, frames, active=None, first=0):
        A = np.zeros((GH, GW, 4), np.float32)
        for chain in self.energy[first:first + frames]:
            A = bake_add(A, self.valid, chain[0], active)
        return A


@pytest.fixture(scope="module")
def floor(oracle_scene):
    f = Floor(oracle_scene)
    assert f.n_valid == GW * GH * 3 // 4
    return f


def device_buffers():
    """The HIP runtime the library itself runs on (already mapped into this process)."""
    with open("/proc/self/maps") as maps:
        hip_path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    hip = C.CDLL(hip_path)
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    return hip


# ---- 1. the floor grid ---------------------------------------------------------------------------------

def test_floor_grid_bitexact(product_scene, floor):
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        assert r.sensor() == (surf_amd.SENSOR_CAMERA, GW * GH)
        r.set_surfel_sensor(floor.pos, floor.nrm)
        assert r.sensor() == (surf_amd.SENSOR_SURFELS, floor.n_valid)
        r.render(4, 0, 0)
        got = r.accumulator()
        assert_acc_equal(got, floor.acc(4), "floor grid, 4 frames")
        inv = ~floor.valid.reshape(GH, GW)
        assert (got[inv].view(np.uint32) == 0).all()                      # all-zero records, w == 0
        assert (got[~inv][:, 3] == F(4.0)).all()
        assert r.stats()["samples"] == 4 * floor.n_valid
        assert floor.info["census"]["diffuse"] > 0 and r.stats()["n_shadow"] > 0      # diffuse bounces, and shadow rays cast from them
        assert r.debug_issue_order() == (0, 0)                            # no permuted head under a sensor
    finally:
        r.close()


# ---- 2. the view as surfels ----------------------------------------------------------------------------

def moved_camera(osc):
    """tests/test_gpu_aov.py::test_misses_after_set_camera's camera: up and back, so that part of the frame is sky."""
    ubo = np.frombuffer(osc.camera_ubo(W, H), np.float32).copy()
    shift = np.array([0.0, 6.0, -12.0], np.float32)
    ubo[0:3] = ubo[0:3] + shift              # position
    ubo[16:19] = ubo[16:19] + shift          # first_pixel
    return ubo.tobytes()


@pytest.mark.parametrize("view", ["bundled", "moved"])
def test_the_view_as_surfels(oracle_scene, product_scene, view):
    """The bundled view (a closed room: every pixel hits, the lens among them) and the moved camera, whose sky pixels are
    invalid texels."""
    ubo = oracle_scene.camera_ubo(W, H) if view == "bundled" else moved_camera(oracle_scene)
    planes, info = expected_planes(oracle_scene, ubo, W, range(H))
    want, valid, vinfo = bake_expected(oracle_scene, planes["position"], planes["normal"], W, range(H), 2, spp=3, max_segments=CAP)
    assert np.array_equal(valid, info["hit"].reshape(-1))                 # a miss is an invalid texel
    if view == "bundled":
        assert vinfo["census"]["dielectric_outside"] >= 1
    else:
        assert not valid.all() and 0.3 <= 1.0 - valid.mean() <= 0.8      # sky pixels: invalid, never issued
        assert (want.reshape(-1, 4)[~valid].view(np.uint32) == 0).all()
    hip = device_buffers()
    r = surf_amd.Renderer(product_scene, W, H, camera=ubo)
    dev = [C.c_void_p(), C.c_void_p()]
    try:
        r.set_zero_cutoff(True)
        r.set_surfel_sensor(planes["position"], planes["normal"])
        r.render(2, 0, CAP, spp=3)
        host = r.accumulator()
        assert_acc_equal(host, want, "the view's first hits from host planes")
        assert r.stats()["samples"] == 6 * int(valid.sum())
        r.set_surfel_sensor(None, None)
        r.clear_accumulator()
        for k in range(2):
            assert hip.hipMalloc(C.byref(dev[k]), W * H * 16) == 0
            r.copy_aov_to(k, dev[k].value)                                # position, normal: no host trip
        r.set_surfel_sensor_device(dev[0].value, dev[1].value)
        assert r.sensor() == (surf_amd.SENSOR_SURFELS, int(valid.sum()))
        for d in dev:                                                     # the library copied them
            hip.hipFree(d)
            d.value = None
        r.render(2, 0, CAP, spp=3)
        device = r.accumulator()
        assert_acc_equal(device, want, "the view's first hits through surf_copy_aov_device")
        assert_acc_equal(device, host, "device planes against host planes")
    finally:
        for d in dev:
            if d.value:
                hip.hipFree(d)
        r.close()


# ---- 3. every engine -----------------------------------------------------------------------------------

@pytest.mark.parametrize("policy,coop,engine", [((0, 8, 4), 0, "lanes"), ((1 << 30, 0, 8), 1 << 30, "coop"), ((1 << 30, 0, 8), 1 << 30, "pair")],
                         ids=["lane-drain", "coop-from-start", "pair-from-start"])
def test_drain_engines(product_scene, floor, policy, coop, engine, monkeypatch):
    monkeypatch.setenv("SURF_TAIL_PAIR", "0" if engine == "coop" else "1")
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        r.set_tail_policy(*policy)
        r.set_tail_coop(coop)
        r.set_surfel_sensor(floor.pos, floor.nrm)
        r.render(2, 0, 0)
        assert_acc_equal(r.accumulator(), floor.acc(2), f"floor grid through the {engine} drain")
        assert r.stats()["samples"] == 2 * floor.n_valid
    finally:
        r.close()


def test_global_tables(floor):
    """Variant 3: 91 instances, so the trace and shading tables are read from global memory."""
    o = oracle.OracleScene(variant=3)
    p = surf_amd.Scene.indoor(variant=3)
    try:
        assert o.instance_count() > 64
        want, _, _ = bake_expected(o, floor.pos, floor.nrm, GW, range(GH), 2)
        r = surf_amd.Renderer(p, GW, GH)
        try:
            r.set_surfel_sensor(floor.pos, floor.nrm)
            r.render(2, 0, 0)
            assert_acc_equal(r.accumulator(), want, "floor grid, variant 3 (global tables)")
        finally:
            r.close()
    finally:
        o.close()
        p.close()


def test_two_level_lane_walk(floor, monkeypatch):
    monkeypatch.setenv("SURF_LANEW", "1")
    p = surf_amd.Scene.indoor()
    try:
        r = surf_amd.Renderer(p, GW, GH)
        try:
            assert r.debug_kernel_selection()["lane_two_level"]
            r.set_surfel_sensor(floor.pos, floor.nrm)
            r.render(2, 0, 0)
            assert_acc_equal(r.accumulator(), floor.acc(2), "floor grid, two-level lane walk")
        finally:
            r.close()
    finally:
        p.close()


# ---- 4. mask interplay ---------------------------------------------------------------------------------

def test_mask_and_validity(product_scene, floor):
    mask = (np.random.default_rng(23).random((GH, GW)) < 0.5).astype(np.uint8)
    valid2 = floor.valid.reshape(GH, GW)
    forced = (mask != 0) & valid2
    assert 0 < forced.sum() < mask.sum()                                  # the mask names invalid texels too
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        r.set_surfel_sensor(floor.pos, floor.nrm)
        m, n = r.pixel_mask()                                             # "no mask" under the sensor: the valid texels
        assert np.array_equal(m != 0, valid2) and n == floor.n_valid
        r.set_pixel_mask(mask)
        m, n = r.pixel_mask()
        assert np.array_equal(m != 0, forced) and n == int(forced.sum())  # the forced bytes
        r.render(3, 0, 0)
        got = r.accumulator()
        assert_acc_equal(got, floor.acc(3, active=forced), "random mask AND valid")
        assert (got[~forced].view(np.uint32) == 0).all()                  # the others: untouched
        assert r.stats()["samples"] == 3 * int(forced.sum())
        r.clear_accumulator()
        m, n = r.pixel_mask()
        assert n == floor.n_valid and np.array_equal(m != 0, valid2)
        r.set_pixel_mask(np.ones((GH, GW), np.uint8))                     # all ones: still only the valid texels
        assert r.pixel_mask()[1] == floor.n_valid
        r.set_pixel_mask(None)
        assert r.pixel_mask()[1] == floor.n_valid
        r.render(2, 0, 0)
        assert_acc_equal(r.accumulator(), floor.acc(2), "after clear_accumulator: every valid texel")
        r.set_surfel_sensor(None, None)                                   # back to the camera: every pixel
        m, n = r.pixel_mask()
        assert m.all() and n == GW * GH
    finally:
        r.close()


def test_last_texel_alone_and_none_at_all(oracle_scene, product_scene, floor):
    nrm = np.zeros((GH, GW, 4), np.float32)
    nrm[-1, -1, 1] = 1.0
    want, valid, _ = bake_expected(oracle_scene, floor.pos, nrm, GW, range(GH), 5)
    assert valid.sum() == 1 and valid[-1]
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        r.set_surfel_sensor(floor.pos, nrm)
        assert r.sensor() == (surf_amd.SENSOR_SURFELS, 1)
        r.render(5, 0, 0)
        assert_acc_equal(r.accumulator(), want, "the last texel alone")
        assert r.stats()["samples"] == 5
        before = r.stats()
        r.set_surfel_sensor(floor.pos, np.zeros((GH, GW, 4), np.float32))          # no valid texel at all
        assert r.sensor() == (surf_amd.SENSOR_SURFELS, 0) and r.pixel_mask()[1] == 0
        assert surf_amd.load().surf_render(r.handle, 3, 5, 0, 1) == 0
        assert_acc_equal(r.accumulator(), want, "a render without a valid texel changes nothing")
        assert r.stats()["samples"] == before["samples"]
        odd = nrm.copy()
        odd[0, 0, 0], odd[0, 1, 2], odd[0, 2, 3] = np.nan, -0.0, 1.0      # NaN: valid; -0 and w alone: not
        r.set_surfel_sensor(floor.pos, odd)
        assert r.sensor() == (surf_amd.SENSOR_SURFELS, 2)
        assert r.pixel_mask()[0].reshape(-1)[[0, 1, 2, -1]].tolist() == [1, 0, 0, 1]
    finally:
        r.close()


# ---- 5. chains and the ring ----------------------------------------------------------------------------

def test_continued_stream_and_the_ring(oracle_scene, product_scene, floor):
    want, _, _ = bake_expected(oracle_scene, floor.pos, floor.nrm, GW, range(GH), 40)
    out = []
    for calls in (40, 1):
        r = surf_amd.Renderer(product_scene, GW, GH, frame_batch=8)
        try:
            r.set_surfel_sensor(floor.pos, floor.nrm)
            for j in range(calls):
                r.render(40 // calls, j, 0)
            out.append(r.accumulator())
            assert r.stats()["frame_window"] == 8                         # 40 passes reuse the 8 slots
            assert r.stats()["samples"] == 40 * floor.n_valid
        finally:
            r.close()
    assert_acc_equal(out[0], out[1], "40 one-frame calls against one 40-frame call")
    assert_acc_equal(out[1], want, "40 frames under the sensor")


@pytest.mark.parametrize("engine", ["wavefront", "coop", "pair", "lanes"])
def test_chains_through_the_drains(oracle_scene, product_scene, floor, engine, monkeypatch):
    """spp = 4: the second to fourth sample of a frame start in k_shade (wavefront to the end) or in the drain kernel that
    ended the one before."""
    want = chained(oracle_scene, floor)
    policy, coop = {"wavefront": ((1, 0, 0), 0), "lanes": ((1 << 30, 8, 4), 0)}.get(engine, ((1 << 30, 0, 8), 1 << 30))
    monkeypatch.setenv("SURF_TAIL_PAIR", "0" if engine == "coop" else "1")
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        r.set_zero_cutoff(True)
        r.set_tail_policy(*policy)
        r.set_tail_coop(coop)
        r.set_surfel_sensor(floor.pos, floor.nrm)
        r.render(2, 0, CAP, spp=4)
        assert_acc_equal(r.accumulator(), want, f"2 frames of 4 chained samples, {engine}")
        assert r.stats()["samples"] == 8 * floor.n_valid
    finally:
        r.close()


_chained = {}


def chained(osc, floor):
    if not _chained:
        _chained["acc"] = bake_expected(osc, floor.pos, floor.nrm, GW, range(GH), 2, spp=4, max_segments=CAP)[0]
        _chained["acc"].setflags(write=False)
    return _chained["acc"]


# ---- 6. row shards -------------------------------------------------------------------------------------

def test_row_shards(product_scene, floor):
    specs = [ShardSpec(k, 2, 1) for k in range(2)]                        # interleaved rows
    parts = []
    for s in specs:
        r = surf_amd.Renderer(product_scene, GW, GH, shard=s)
        try:
            assert len(r.rows) == GH // 2
            r.set_surfel_sensor(floor.pos[r.rows], floor.nrm[r.rows])     # each context takes its own rows' planes
            assert r.sensor()[1] == int(floor.valid.reshape(GH, GW)[r.rows].sum())
            r.render(3, 0, 0)
            parts.append(r.accumulator())
        finally:
            r.close()
    assert_acc_equal(surf_amd.assemble_shards(GW, GH, parts, specs), floor.acc(3), "two interleaved row shards")


# ---- 7. switching back -----------------------------------------------------------------------------------

def test_switching_back_to_the_camera(oracle_scene, product_scene, floor):
    oracle.set_zero_cutoff(True)
    try:
        want, cnt, _ = oracle_scene.render(GW, GH, 3)
    finally:
        oracle.set_zero_cutoff(False)
    plain = surf_amd.Renderer(product_scene, GW, GH)
    try:
        plain.render(3, 0, 0)
        never, st_never = plain.accumulator(), plain.stats()
    finally:
        plain.close()
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        r.set_surfel_sensor(floor.pos, floor.nrm)
        r.render(2, 0, 0)
        assert_acc_equal(r.accumulator(), floor.acc(2), "the bake before the switch")
        r.set_surfel_sensor(None, None)
        assert r.sensor() == (surf_amd.SENSOR_CAMERA, GW * GH)
        r.clear_accumulator()
        r.render(3, 0, 0)
        back, st = r.accumulator(), r.stats()
    finally:
        r.close()
    assert_acc_equal(back, want, "the camera render after a sensor, against the oracle")
    assert_acc_equal(back, never, "... and against a context that never had a sensor")
    for k in ("samples", "n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc"):
        assert st[k] == st_never[k], k
    assert [st[k] for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")] == [cnt[k] for k in
                                                                                              ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")]


def test_sensor_survives_camera_and_instance_updates(floor):
    o = oracle.OracleScene()
    p = surf_amd.Scene.indoor()
    try:
        r = surf_amd.Renderer(p, GW, GH)
        try:
            r.set_surfel_sensor(floor.pos, floor.nrm)
            ubo = np.frombuffer(p.camera(GW, GH), np.float32).copy()
            ubo[0:3] += np.array([0.0, 1.0, -2.0], np.float32)            # another camera: the points are world-space data
            r.set_camera(ubo.tobytes())
            o.update(0.5)
            p.update(0.5)
            r.update_instances(p)
            assert r.sensor() == (surf_amd.SENSOR_SURFELS, floor.n_valid)
            want, _, _ = bake_expected(o, floor.pos, floor.nrm, GW, range(GH), 2)
            assert not np.array_equal(want.view(np.uint32), floor.acc(2).view(np.uint32)), "the update changed nothing the grid sees"
            r.render(2, 0, 0)
            assert_acc_equal(r.accumulator(), want, "the bake on the updated scene")
        finally:
            r.close()
    finally:
        o.close()
        p.close()


# ---- 8. downstream on a light map ------------------------------------------------------------------------

LOOP = dict(threshold=0.5, floor=0.01, min_samples=4, max_samples=8, dilate=1, batch=4)


def np_adaptive_valid(frames, valid2, **p):
    """tests/test_adaptive_host.py's np_adaptive with the invalid texels never active: "every pixel" is every valid texel
    and each built mask is ANDed with the validity before it is used."""
    mp = {k: p[k] for k in ("threshold", "floor", "min_samples", "max_samples", "dilate")}
    h, w = valid2.shape
    A, Q = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    for j in range(p["min_samples"]):
        A, Q = np_add_frame(A, Q, frames[j], valid2.astype(np.uint8))
    f, total, round_active = p["min_samples"], p["min_samples"] * int(valid2.sum()), []
    while True:
        mask = np_mask(A, Q, **mp)[0] & valid2.astype(np.uint8)
        n = int(mask.sum())
        if n == 0 or f == p["max_samples"]:
            break
        nb = min(p["batch"], p["max_samples"] - f)
        round_active.append(n)
        for j in range(nb):
            A, Q = np_add_frame(A, Q, frames[f + j], mask)
        total += nb * n
        f += nb
    return {"acc": A, "squares": Q, "mask": mask, "round_active": round_active, "frames": f, "samples": total, "active_last": n}


def test_downstream_on_a_light_map(product_scene, floor):
    valid2 = floor.valid.reshape(GH, GW)
    want = np_adaptive_valid(frame_planes(floor.valid, floor.energy, (GH, GW, 4)), valid2, **LOOP)
    assert want["round_active"] and 0 < want["round_active"][0] <= floor.n_valid
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        r.set_sample_squares(True)
        r.set_sample_buckets(4)
        r.set_surfel_sensor(floor.pos, floor.nrm)
        got = r.render_adaptive(**LOOP)
        assert got["round_active"] == want["round_active"], (got["round_active"], want["round_active"])
        assert (got["frames"], got["samples"], got["active_last"]) == (want["frames"], want["samples"], want["active_last"])
        acc = r.accumulator()
        assert_acc_equal(acc, want["acc"], "render_adaptive on the light map: accumulator")
        assert_acc_equal(r.sample_squares(), want["squares"], "render_adaptive on the light map: squares")
        m, n = r.pixel_mask()
        assert np.array_equal(m, want["mask"]) and n == want["active_last"]
        assert (acc[~valid2].view(np.uint32) == 0).all() and r.stats()["samples"] == want["samples"]
        buckets = r.sample_buckets()
        assert (buckets[:, ~valid2].view(np.uint32) == 0).all()
        total = buckets[0] + buckets[1] + buckets[2] + buckets[3]
        assert np.array_equal(total[..., 3], acc[..., 3])
        out, trim, summary = r.robust()
        h_out, h_trim, h_summary = surf_amd.robust_image_host(acc, buckets)
        assert_acc_equal(out, h_out, "robust() on the light map against its host twin")
        assert np.array_equal(trim, h_trim.reshape(trim.shape)) and summary == h_summary
        img, err = r.denoise_nlm(search_radius=3, patch_radius=1)
        h_img, h_err = surf_amd.denoise_nlm_image_host(*np_halves(buckets), search_radius=3, patch_radius=1)
        assert_acc_equal(img, h_img, "denoise_nlm() on the light map against its host twin")
        assert_acc_equal(err, h_err, "denoise_nlm()'s error estimate against its host twin")
    finally:
        r.close()


# ---- 9. refusals and the example -------------------------------------------------------------------------

def test_status_codes(product_scene, floor):
    lib = surf_amd.load()
    h = C.c_void_p()
    pos, nrm = np.ascontiguousarray(floor.pos[:8, :8]), np.ascontiguousarray(floor.nrm[:8, :8])
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        k, v = C.c_int(), C.c_uint32()
        assert lib.surf_set_surfel_sensor(h, pos.ctypes.data, None) == SURF_ERR_INVALID
        assert lib.surf_set_surfel_sensor(h, None, nrm.ctypes.data) == SURF_ERR_INVALID
        assert lib.surf_set_surfel_sensor_device(h, None, nrm.ctypes.data) == SURF_ERR_INVALID
        assert b"NULL" in lib.surf_last_error(h)
        assert lib.surf_get_sensor(h, C.byref(k), C.byref(v)) == 0 and (k.value, v.value) == (0, 64)
        assert lib.surf_set_surfel_sensor(h, pos.ctypes.data, nrm.ctypes.data) == 0      # needs no scene and no camera ...
        assert lib.surf_get_sensor(h, C.byref(k), None) == 0 and k.value == 1
        assert lib.surf_get_sensor(h, None, C.byref(v)) == 0 and v.value == int(valid_texels(nrm).sum())
        assert lib.surf_render(h, 1, 0, 0, 1) == SURF_ERR_NO_SCENE                        # ... surf_render still does
        tiny = nrm.copy()
        tiny[3, 3, :3] = (0.0, 1e-25, 0.0)                                               # nonzero, squared length underflows: refused,
        assert lib.surf_set_surfel_sensor(h, pos.ctypes.data, tiny.ctypes.data) == SURF_ERR_INVALID
        assert b"underflows" in lib.surf_last_error(h)
        assert lib.surf_get_sensor(h, C.byref(k), C.byref(v)) == 0 and (k.value, v.value) == (1, int(valid_texels(nrm).sum()))   # nothing changed
        assert lib.surf_set_surfel_sensor(h, None, None) == 0
        assert lib.surf_get_sensor(h, C.byref(k), C.byref(v)) == 0 and (k.value, v.value) == (0, 64)
    finally:
        lib.surf_destroy(h)
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        acc = r.bake(floor.pos, floor.nrm, 2)                             # Renderer.bake: set, clear, render, read, restore
        assert_acc_equal(acc, floor.acc(2), "Renderer.bake")
        assert r.sensor() == (surf_amd.SENSOR_CAMERA, GW * GH)
        assert_acc_equal(r.bake(floor.pos, floor.nrm, 2, first_sample=2), floor.acc(2, first=2), "Renderer.bake from sample 2")
    finally:
        r.close()


def mean_image(acc):
    with np.errstate(all="ignore"):
        return np.where(acc[..., 3:] > 0, acc[..., :3] / acc[..., 3:], F(0.0)).astype(np.float32)


def test_cpp_example_matches_python(product_scene, tmp_path):
    exe = os.path.join(surf_amd._PKG, "build", "render_baked")
    prefix = str(tmp_path / "baked")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(GW), str(GH), "2"] + [repr(float(v)) for v in FLOOR] + [prefix],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    pos, nrm = floor_grid(GW, GH, *FLOOR)
    r = surf_amd.Renderer(product_scene, GW, GH)
    try:
        planes = r.aov()
        view = r.bake(planes["position"], planes["normal"], 2)
        grid = r.bake(pos, nrm, 2)
    finally:
        r.close()
    for name, acc in (("view", view), ("floor", grid)):
        pfm = np.ascontiguousarray(read_pfm(f"{prefix}_{name}.pfm"))
        assert np.array_equal(pfm.view(np.uint32), np.ascontiguousarray(mean_image(acc)).view(np.uint32)), name
        with open(f"{prefix}_{name}.png", "rb") as f:
            assert f.read(8) == b"\x89PNG\r\n\x1a\n"
    assert (grid[..., 3] == F(2.0)).all()
