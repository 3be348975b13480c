"""First-hit feature buffers (AOVs, surf_read_aov / Renderer.aov()) against the
CPU oracle plus numpy.

Bar: bit-exact.  The expected planes never come from the code under test: the
camera rays are rebuilt here in numpy from the 128-byte camera UBO, traced by
the oracle (oracle_scene.trace_closest), and the planes are computed from the
oracle's scene export, every step an explicit float32 operation in the order
include/surf_hip.h states.  numpy's float32 add / multiply / divide / sqrt are
single IEEE operations (no contraction), as the kernels are built.  Planes
are compared as uint32 words.

All frames are 100 x 37: 3,700 pixels, no multiple of the 256-lane block, so
the last block is partial.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import surf_amd

pytestmark = pytest.mark.gpu
UNSET = 0xFFFFFFFF
F = np.float32
W, H = 100, 37
PLANES = surf_amd.AOV_PLANES


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


# ---- the expected planes (oracle + numpy float32) ---------------------------

def camera_rays(ubo: bytes, width: int, rows):
    """The unjittered camera ray of every pixel of `rows` (no lens sample)."""
    c = np.frombuffer(ubo, np.float32)
    pos, first, uvec, vvec, res = c[0:3], c[16:19], c[20:23], c[24:27], c[28:30]
    inv_w, inv_h = F(1.0) / res[0], F(1.0) / res[1]
    rows = np.asarray(rows, np.uint32)
    x = np.tile(np.arange(width, dtype=np.uint32), len(rows)).astype(np.float32)
    row = np.repeat(rows, width).astype(np.float32)
    u, v = x * inv_w, row * inv_h
    dirs = [((first[a] + u * uvec[a]) + v * vvec[a]) - pos[a] for a in range(3)]
    len2 = ((F(0.0) + dirs[0] * dirs[0]) + dirs[1] * dirs[1]) + dirs[2] * dirs[2]
    inv = F(1.0) / np.sqrt(len2)
    d = np.stack([dirs[a] * inv for a in range(3)], axis=1)
    o = np.broadcast_to(pos, d.shape).copy()
    assert o.dtype == np.float32 and d.dtype == np.float32
    return o, d


def expected_planes(osc, ubo: bytes, width: int, rows):
    """(planes, info): the four planes as (len(rows), width, 4) arrays, and what
    the frame exercises (hit mask, instance ids, flipped normals, emitters)."""
    o, d = camera_rays(ubo, width, rows)
    t, u, v, inst, prim = osc.trace_closest(o, d)
    ex = osc.export()
    inst_u = np.frombuffer(ex["instances"], np.uint32).reshape(-1, 40)    # tri_offset @0, material_offset @12
    inst_f = np.frombuffer(ex["instances"], np.float32).reshape(-1, 40)   # M column-major @32
    text = np.frombuffer(ex["tri_ext"], np.float32).reshape(-1, 20)       # n0 @0, n1 @16, n2 @32
    mats = np.frombuffer(ex["materials"], np.float32).reshape(-1, 16)     # strength @0, emission @16, albedo @32
    bg_u = np.frombuffer(ex["background"], np.uint32)
    bg_f = np.frombuffer(ex["background"], np.float32)                    # color @16, gradient A @32, B @48
    n = len(t)
    hit = inst != UNSET
    ii, pp = np.where(hit, inst, 0), np.where(hit, prim, 0)
    tri = inst_u[ii, 0] + pp
    mat = inst_u[ii, 3]
    col = lambda a: a[:, None]
    with np.errstate(all="ignore"):                                       # miss lanes compute discarded values
        # position: (o + t d, t)
        P = o + col(t) * d
        # normal: M (u n0 + v n2 + w n1, 0), normalized as a vec4, turned against d
        n0, n1, n2 = text[tri, 0:3], text[tri, 4:7], text[tri, 8:11]
        w = (F(1.0) - u) - v
        no = (col(u) * n0 + col(v) * n2) + col(w) * n1
        M = inst_f[ii, 8:24]
        mrow = lambda i: (M[:, i] * no[:, 0] + M[:, 4 + i] * no[:, 1]) + (M[:, 8 + i] * no[:, 2] + M[:, 12 + i] * F(0.0))
        nx, ny, nz, nw = mrow(0), mrow(1), mrow(2), mrow(3)
        nn = (nx * nx + ny * ny) + (nz * nz + nw * nw)
        ninv = F(1.0) / np.sqrt(nn)
        N = np.stack([nx * ninv, ny * ninv, nz * ninv], axis=1)
        flip = ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]) > F(0.0)
        N = np.where(col(flip), N * F(-1.0), N)
        # albedo: emitters show strength * colour
        strength, ecol = mats[mat, 0], mats[mat, 4:7]
        emitter = (strength > F(0.0)) & ((ecol[:, 0] > F(0.0)) | (ecol[:, 1] > F(0.0)) | (ecol[:, 2] > F(0.0)))
        A = np.where(col(emitter), col(strength) * ecol, mats[mat, 8:11])
        # background along d for the misses
        bg = np.zeros((n, 3), np.float32)
        if bg_u[0] == 0:
            bg[:] = bg_f[4:7]
        elif bg_u[0] == 1:
            a = F(0.5) * (F(1.0) + d[:, 1])
            bg = col(a) * bg_f[12:15] + col(F(1.0) - a) * bg_f[8:11]
    for arr in (P, N, A, bg):
        assert arr.dtype == np.float32
    zero, one = np.zeros(n, np.float32), np.ones(n, np.float32)
    pos = np.where(col(hit), np.column_stack([P, t]), np.column_stack([zero, zero, zero, np.full(n, 1e30, np.float32)]))
    nrm = np.where(col(hit), np.column_stack([N, zero]), F(0.0))
    alb = np.where(col(hit), np.column_stack([A, one]), np.column_stack([bg, zero]))
    ids = np.where(col(hit), np.column_stack([inst, prim, mat, np.zeros(n, np.uint32)]),
                   np.array([UNSET, UNSET, UNSET, 0], np.uint32)).astype(np.uint32)
    shape = (len(rows), width, 4)
    planes = {"position": pos.astype(np.float32).reshape(shape), "normal": nrm.astype(np.float32).reshape(shape),
              "albedo": alb.astype(np.float32).reshape(shape), "id": ids.reshape(shape)}
    info = {"hit": hit, "inst": inst, "flip": flip & hit, "emitter": emitter & hit, "gradient": bg_u[0] == 1}
    return planes, info


def assert_planes_equal(got, want, what):
    for name in PLANES:
        g, w = got[name], want[name]
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what} {name}: {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert len(bad) == 0, (f"{what}: plane {name}: {len(bad)} words differ, first (row, x, channel) {bad[:4].tolist()}: "
                               f"got {g[tuple(bad[0])]!r}, want {w[tuple(bad[0])]!r}")


@pytest.fixture(scope="module")
def indoor_expected(oracle_scene):
    """Expected planes of the bundled scene's default 100 x 37 view (shared, read only)."""
    planes, info = expected_planes(oracle_scene, oracle_scene.camera_ubo(W, H), W, range(H))
    for a in planes.values():
        a.setflags(write=False)
    return planes, info


# ---- 1. indoor view: LDS tables, global tables, the two-level lane walk ------

def test_indoor_planes_bitexact(oracle_scene, product_scene, indoor_expected):
    want, info = indoor_expected
    hit = info["hit"]
    # the frame exercises the branches (oracle side): several instances, an emitter, flipped normals
    assert len(np.unique(info["inst"][hit])) >= 5
    assert info["emitter"].sum() >= 1
    assert info["flip"].sum() >= 0.2 * hit.sum()
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        got = r.aov()
        assert_planes_equal(got, want, "indoor variant 0")
        again = r.aov()                      # the cached planes
        assert_planes_equal(again, got, "second read")
    finally:
        r.close()


def test_indoor_planes_two_level_lane_walk(oracle_scene, indoor_expected, monkeypatch):
    """The laneW kernel variant (two-level records, forced on the bundled scene)."""
    monkeypatch.setenv("SURF_LANEW", "1")
    p = surf_amd.Scene.indoor()
    try:
        r = surf_amd.Renderer(p, W, H)
        assert_planes_equal(r.aov(), indoor_expected[0], "indoor variant 0, two-level lane walk")
        r.close()
    finally:
        p.close()


def test_global_tables_planes_bitexact():
    """Variant 3: 91 instances, so the trace and shading tables are read from
    global memory, and the TLAS has interior nodes."""
    o = oracle.OracleScene(variant=3)
    p = surf_amd.Scene.indoor(variant=3)
    try:
        assert o.instance_count() > 64
        want, info = expected_planes(o, o.camera_ubo(W, H), W, range(H))
        assert (info["inst"][info["hit"]] >= 64).sum() >= 1, "no pixel sees an instance past the LDS table size"
        r = surf_amd.Renderer(p, W, H)
        assert_planes_equal(r.aov(), want, "variant 3 (global tables)")
        r.close()
    finally:
        o.close()
        p.close()


# ---- 2. misses, through set_camera (the cache is dropped) ---------------------

def test_misses_after_set_camera(oracle_scene, product_scene, indoor_expected):
    ubo = np.frombuffer(oracle_scene.camera_ubo(W, H), np.float32).copy()
    shift = np.array([0.0, 6.0, -12.0], np.float32)
    ubo[0:3] = ubo[0:3] + shift              # position
    ubo[16:19] = ubo[16:19] + shift          # first_pixel
    moved = ubo.tobytes()
    want, info = expected_planes(oracle_scene, moved, W, range(H))
    miss = 1.0 - info["hit"].mean()
    assert 0.3 <= miss <= 0.8, f"{miss:.3f} of the pixels miss"
    assert info["gradient"], "the bundled scene's background is a gradient"
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        before = r.aov()                     # default camera: fills the cache
        assert_planes_equal(before, indoor_expected[0], "default camera")
        r.set_camera(moved)
        got = r.aov()
        assert_planes_equal(got, want, "moved camera")
        m = ~info["hit"].reshape(H, W)
        assert (got["albedo"][m][:, 3] == 0.0).all() and (got["position"][m][:, 3] == F(1e30)).all()
        assert (got["id"][m][:, :3] == UNSET).all()
    finally:
        r.close()


# ---- 3. animation: update_instances drops the cache ---------------------------

def test_planes_follow_instance_update():
    o = oracle.OracleScene()
    p = surf_amd.Scene.indoor()
    try:
        ubo = o.camera_ubo(W, H)
        r = surf_amd.Renderer(p, W, H)
        before = r.aov()
        assert_planes_equal(before, expected_planes(o, ubo, W, range(H))[0], "before the update")
        o.update(0.5)
        p.update(0.5)
        r.update_instances(p)
        want, _ = expected_planes(o, ubo, W, range(H))
        got = r.aov()
        assert_planes_equal(got, want, "after update(0.5)")
        assert (want["id"] != before["id"]).any(axis=-1).sum() > 0, "the update moved nothing in view"
        assert not np.array_equal(got["id"], before["id"])
        r.close()
    finally:
        o.close()
        p.close()


# ---- 4. row shards ------------------------------------------------------------

def test_row_shards_assemble_to_the_frame(product_scene):
    specs = [surf_amd.ShardSpec(k, 3, 2) for k in range(3)]          # 19 row blocks, the last a single row
    whole = surf_amd.Renderer(product_scene, W, H)
    full = whole.aov()
    whole.close()
    parts = []
    for s in specs:
        r = surf_amd.Renderer(product_scene, W, H, shard=s)
        parts.append(r.aov())
        r.close()
    assert sorted(len(p["id"]) for p in parts) == [12, 12, 13]
    for name in PLANES:
        # assemble_shards places float32 rows: the id plane travels as a float32 view of its bits
        got = surf_amd.assemble_shards(W, H, [p[name].view(np.float32) for p in parts], specs)
        assert np.array_equal(got.view(np.uint32), full[name].view(np.uint32)), name


# ---- 5. a read in the middle of a sample stream changes nothing ---------------

def test_read_is_neutral_to_the_sample_stream(product_scene):
    w, h = 32, 24
    out = []
    for read in (True, False):
        r = surf_amd.Renderer(product_scene, w, h)
        r.render(2, 0)
        if read:
            planes = r.aov()
            assert (planes["id"][..., 0] != UNSET).any()
        r.render(2, 2)
        out.append((r.accumulator(), r.stats()))
        r.close()
    (acc_a, st_a), (acc_b, st_b) = out
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc", "samples"):
        assert st_a[k] == st_b[k], k
    assert st_a["samples"] == 4 * w * h


# ---- 6. the C++ API and the example -------------------------------------------

def read_pfm(path):
    blob = open(path, "rb").read()
    magic, dims, scale, data = blob.split(b"\n", 3)
    w, h = (int(x) for x in dims.split())
    assert magic == b"PF" and scale == b"-1.0"
    return np.frombuffer(data, "<f4").reshape(h, w, 3)[::-1]         # rows bottom to top in the file


def test_cpp_example_matches_python(product_scene, tmp_path):
    w, h = 64, 48
    exe = os.path.join(surf_amd._PKG, "build", "render_aov")
    prefix = str(tmp_path / "aov")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(w), str(h), prefix], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = surf_amd.Renderer(product_scene, w, h)
    want = r.aov()
    r.close()
    raw = np.fromfile(prefix + "_planes.bin", np.uint32)
    assert raw.size == 4 * w * h * 4
    raw = raw.reshape(4, h, w, 4)
    for k, name in enumerate(PLANES):
        assert np.array_equal(raw[k], want[name].view(np.uint32)), name
    pfm = read_pfm(prefix + "_normal.pfm")
    assert np.array_equal(np.ascontiguousarray(pfm).view(np.uint32), np.ascontiguousarray(want["normal"][..., :3]).view(np.uint32))
    for name in ("position", "albedo"):
        assert os.path.getsize(f"{prefix}_{name}.pfm") == len(f"PF\n{w} {h}\n-1.0\n") + w * h * 12


# ---- 7. status codes and the device-to-device copy ----------------------------

def test_status_codes_and_device_copy(product_scene):
    lib = surf_amd.load()
    buf = np.zeros((8, 8, 4), np.float32)
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        assert lib.surf_read_aov(h, 0, buf.ctypes.data) == -4            # SURF_ERR_NO_SCENE: nothing uploaded
        assert lib.surf_read_aov(h, 4, buf.ctypes.data) == -1            # SURF_ERR_INVALID: planes are 0..3
        assert lib.surf_read_aov(h, -1, buf.ctypes.data) == -1
        assert lib.surf_read_aov(h, 0, None) == -1
        assert lib.surf_copy_aov_device(h, 0, None) == -1
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
        want = r.aov()
        assert hip.hipMalloc(C.byref(dev), W * H * 16) == 0
        for k, name in enumerate(PLANES):
            r.copy_aov_to(k, dev.value)
            got = np.zeros((H, W, 4), np.uint32)
            assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0   # hipMemcpyDeviceToHost
            assert np.array_equal(got, want[name].view(np.uint32)), name
    finally:
        if dev.value:
            hip.hipFree(dev)
        r.close()
