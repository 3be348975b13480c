"""Feature buffers traced through mirrors and glass (surf_read_aov_chain /
Renderer.aov_chain()) against the CPU oracle plus numpy.

Bar: bit-exact.  The expected planes never come from the code under test:
chain_planes below restates the chain include/surf_hip.h defines, every step
an explicit float32 numpy operation in the stated order, with the oracle's
closest-hit traversal (oracle_scene.trace_closest) once per link on the pixels
still active and glibc's expf through ctypes for the absorption
(tests/test_libm.py pins the library's gExpf to glibc).  Planes are compared as
uint32 words.

All frames are 100 x 37, the view of tests/test_gpu_aov.py.

One branch has no case here: the tinted miss after at least one link.  The
bundled room is closed, so no view of it reaches that branch; its case is in
tests/test_gpu_scene_edges.py, where an edited scene opens the room.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import surf_amd
from test_denoise_host import glibc_expf
from test_gpu_aov import UNSET, W, H, assert_planes_equal, camera_rays, expected_planes, read_pfm

pytestmark = pytest.mark.gpu
F = np.float32
PLANES = surf_amd.AOV_PLANES
K_EPS = F(1e-5)


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


# ---- the expected planes (oracle + numpy float32) ---------------------------

def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def chain_planes(osc, ubo: bytes, width: int, rows, max_links: int):
    """(planes, info): the four chain planes as (len(rows), width, 4) arrays, and
    per pixel what its chain did (links, reflect / refract / TIR links taken,
    how it ended)."""
    o_all, d_all = camera_rays(ubo, width, rows)
    ex = osc.export()
    inst_u = np.frombuffer(ex["instances"], np.uint32).reshape(-1, 40)    # tri_offset @0, material_offset @12
    inst_f = np.frombuffer(ex["instances"], np.float32).reshape(-1, 40)   # M column-major @32
    text = np.frombuffer(ex["tri_ext"], np.float32).reshape(-1, 20)       # n0 @0, n1 @16, n2 @32
    mats = np.frombuffer(ex["materials"], np.float32).reshape(-1, 16)     # strength, refl, refr, ior, emission @16, albedo @32, absorption @48
    bg_u = np.frombuffer(ex["background"], np.uint32)
    bg_f = np.frombuffer(ex["background"], np.float32)                    # color @16, gradient A @32, B @48
    n = len(o_all)
    col = lambda a: a[:, None]
    pos = np.tile(np.array([0, 0, 0, 1e30], np.float32), (n, 1))
    nrm = np.zeros((n, 4), np.float32)
    alb = np.zeros((n, 4), np.float32)
    ids = np.tile(np.array([UNSET, UNSET, UNSET, 0], np.uint32), (n, 1))
    info = {k: np.zeros(n, np.uint32) for k in ("reflect", "refract", "tir", "tir_outside")}
    info.update({k: np.zeros(n, bool) for k in ("exhausted", "ended_in_medium", "ended_after_exit", "ended_miss", "ended_emitter")})
    # the state of the pixels still active
    act = np.arange(n)
    o, d = o_all.copy(), d_all.copy()
    tint = np.ones((n, 3), np.float32)
    L = np.zeros(n, np.float32)
    in_medium = np.zeros(n, bool)
    just_exited = np.zeros(n, bool)
    for k in range(max_links + 1):
        if len(act) == 0:
            break
        t, u, v, inst, prim = osc.trace_closest(o, d)
        hit = inst != UNSET
        # 1. terminal miss: (tint * background along the last d, 0)
        if (~hit).any():
            m = ~hit
            dm = d[m]
            bg = np.zeros((m.sum(), 3), np.float32)
            if bg_u[0] == 0:
                bg[:] = bg_f[4:7]
            elif bg_u[0] == 1:
                a = F(0.5) * (F(1.0) + dm[:, 1])
                bg = col(a) * bg_f[12:15] + col(F(1.0) - a) * bg_f[8:11]
            c = tint[m] * bg
            assert c.dtype == np.float32
            alb[act[m]] = np.column_stack([c, np.zeros(m.sum(), np.float32)])
            ids[act[m], 3] = k
            info["ended_miss"][act[m]] = True
        # the hits go on
        act, o, d, tint, L, in_medium, just_exited = (x[hit] for x in (act, o, d, tint, L, in_medium, just_exited))
        t, u, v, inst, prim = (x[hit] for x in (t, u, v, inst, prim))
        if len(act) == 0:
            break
        tri = inst_u[inst, 0] + prim
        mat = inst_u[inst, 3]
        M = mats[mat]
        strength, refl, refr, ior = M[:, 0], M[:, 1], M[:, 2], M[:, 3]
        ecol, albedo, absorb = M[:, 4:7], M[:, 8:11], M[:, 12:15]
        # 2. the emitter test
        emitter = (strength > F(0.0)) & ((ecol[:, 0] > F(0.0)) | (ecol[:, 1] > F(0.0)) | (ecol[:, 2] > F(0.0)))
        # 3. the hit
        L = L + t
        nd = -t
        absorbing = in_medium & ~emitter
        medium = np.ones((len(act), 3), np.float32)
        if absorbing.any():
            medium[absorbing] = glibc_expf(absorb[absorbing] * col(nd[absorbing]))
        P = o + col(t) * d
        n0, n1, n2 = text[tri, 0:3], text[tri, 4:7], text[tri, 8:11]
        w = (F(1.0) - u) - v
        no = (col(u) * n0 + col(v) * n2) + col(w) * n1
        Mi = inst_f[inst, 8:24]
        mrow = lambda i: (Mi[:, i] * no[:, 0] + Mi[:, 4 + i] * no[:, 1]) + (Mi[:, 8 + i] * no[:, 2] + Mi[:, 12 + i] * F(0.0))
        nx, ny, nz, nw = mrow(0), mrow(1), mrow(2), mrow(3)
        nn = (nx * nx + ny * ny) + (nz * nz + nw * nw)
        ninv = F(1.0) / np.sqrt(nn)
        N = np.stack([nx * ninv, ny * ninv, nz * ninv], axis=1)
        flip = dot3(d, N) > F(0.0)
        N = np.where(col(flip), N * F(-1.0), N)
        # 4. terminal surface: an emitter, a surface that is not delta, or the last link
        delta = (refl + refr) >= F(0.5)
        last = np.full(len(act), k == max_links)
        term = emitter | ~delta | last
        a = np.where(col(emitter), col(strength) * ecol, albedo)
        c = (tint * medium) * a
        for arr in (L, P, N, c, medium):
            assert arr.dtype == np.float32
        tm = act[term]
        pos[tm] = np.column_stack([P, L])[term]
        nrm[tm] = np.column_stack([N, np.zeros(len(act), np.float32)])[term]
        alb[tm] = np.column_stack([c, np.ones(len(act), np.float32)])[term]
        ids[tm] = np.column_stack([inst, prim, mat, np.full(len(act), k, np.uint32)]).astype(np.uint32)[term]
        info["exhausted"][tm] = (delta & ~emitter)[term]
        info["ended_in_medium"][tm] = in_medium[term]
        info["ended_after_exit"][tm] = just_exited[term]
        info["ended_emitter"][tm] = emitter[term]
        # 5. the link
        go = ~term
        tint = tint * (albedo * medium)
        dn = dot3(N, d)
        R = d - col(F(2.0) * dn) * N
        dielectric = ~(refl >= refr)
        n1f = np.where(in_medium, ior, F(1.0)).astype(np.float32)
        n2f = np.where(in_medium, F(1.0), ior).astype(np.float32)
        ratio = n1f / n2f
        cos_i = -dot3(d, N)
        cos2 = F(1.0) - (ratio * ratio) * (F(1.0) - cos_i * cos_i)
        refract = dielectric & (cos2 > F(0.0))
        Rt = col(ratio) * d + col(ratio * cos_i - np.sqrt(np.abs(cos2))) * N
        R = np.where(col(refract), Rt, R)
        for arr in (tint, R, ratio, cos2):
            assert arr.dtype == np.float32
        info["reflect"][act[go & ~dielectric]] += 1
        info["refract"][act[go & refract]] += 1
        info["tir"][act[go & dielectric & ~refract]] += 1
        info["tir_outside"][act[go & dielectric & ~refract & ~in_medium]] += 1      # an ior below 1: no bundled material
        just_exited = refract & in_medium
        in_medium = np.where(refract, ~in_medium, in_medium)
        # 6. advance
        o = P + K_EPS * R
        d = R
        act, o, d, tint, L, in_medium, just_exited = (x[go] for x in (act, o, d, tint, L, in_medium, just_exited))
        o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    assert len(act) == 0
    info["links"] = ids[:, 3].copy()
    shape = (len(rows), width, 4)
    planes = {"position": pos.reshape(shape), "normal": nrm.reshape(shape), "albedo": alb.reshape(shape), "id": ids.reshape(shape)}
    return planes, info


def frozen(planes_info):
    for a in planes_info[0].values():
        a.setflags(write=False)
    return planes_info


@pytest.fixture(scope="module")
def chain8(oracle_scene):
    return frozen(chain_planes(oracle_scene, oracle_scene.camera_ubo(W, H), W, range(H), 8))


@pytest.fixture(scope="module")
def chain2(oracle_scene):
    return frozen(chain_planes(oracle_scene, oracle_scene.camera_ubo(W, H), W, range(H), 2))


@pytest.fixture(scope="module")
def first_hit(oracle_scene):
    return frozen(expected_planes(oracle_scene, oracle_scene.camera_ubo(W, H), W, range(H)))


# ---- 1. / 2. the indoor view at 8 and at 2 links -------------------------------

def test_chain_8_links_bitexact(product_scene, chain8):
    want, info = chain8
    links = info["links"]
    # the frame exercises the branches (oracle side)
    assert (links >= 1).sum() >= 60, (links >= 1).sum()
    assert (links >= 2).sum() >= 20, (links >= 2).sum()
    assert (info["tir"] >= 1).sum() >= 10, (info["tir"] >= 1).sum()
    assert (info["reflect"] >= 1).any() and (info["refract"] >= 1).any()
    assert info["ended_after_exit"].sum() >= 1
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        got = r.aov_chain(8)
        assert_planes_equal(got, want, "8 links")
        assert_planes_equal(r.aov_chain(8), got, "second read")
        assert r.debug_aov_chain_time() > 0.0
    finally:
        r.close()


def test_chain_2_links_bitexact(product_scene, chain2):
    want, info = chain2
    assert info["exhausted"].sum() >= 10, info["exhausted"].sum()
    assert (info["exhausted"] & info["ended_in_medium"]).sum() >= 1, "no terminal applies the absorption"
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert_planes_equal(r.aov_chain(2), want, "2 links")
    finally:
        r.close()


# ---- 3. zero links are the first-hit planes; so is every pixel that is not delta

def test_zero_links_equal_aov_and_non_delta_pixels_keep_their_record(oracle_scene, product_scene, first_hit):
    mats = np.frombuffer(oracle_scene.export()["materials"], np.float32).reshape(-1, 16)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        aov = r.aov()
        assert_planes_equal(aov, first_hit[0], "first-hit planes")
        assert_planes_equal(r.aov_chain(0), aov, "0 links")
        got = r.aov_chain(8)
    finally:
        r.close()
    hit = aov["id"][..., 0] != UNSET
    mat = np.where(hit, aov["id"][..., 2], 0)
    delta = hit & ((mats[mat, 1] + mats[mat, 2]) >= F(0.5))
    assert delta.sum() >= 60 and (~delta).sum() >= 1000
    for name in PLANES:
        assert np.array_equal(got[name][~delta].view(np.uint32), aov[name][~delta].view(np.uint32)), name
    assert (got["id"][delta][:, 3] >= 1).all() and (got["id"][~delta][:, 3] == 0).all()


# ---- 4. both walk variants -----------------------------------------------------

def test_chain_two_level_lane_walk(chain8, monkeypatch):
    """The laneW kernel variant (two-level records, forced on the bundled scene)."""
    monkeypatch.setenv("SURF_LANEW", "1")
    p = surf_amd.Scene.indoor()
    try:
        r = surf_amd.Renderer(p, W, H)
        assert_planes_equal(r.aov_chain(8), chain8[0], "8 links, two-level lane walk")
        r.close()
    finally:
        p.close()


def test_chain_global_tables():
    """Variant 3: 91 instances, so the trace and shading tables are read from
    global memory, and the TLAS has interior nodes."""
    o = oracle.OracleScene(variant=3)
    p = surf_amd.Scene.indoor(variant=3)
    try:
        assert o.instance_count() > 64
        want, info = chain_planes(o, o.camera_ubo(W, H), W, range(H), 8)
        assert (info["links"] >= 1).sum() >= 60
        r = surf_amd.Renderer(p, W, H)
        assert_planes_equal(r.aov_chain(8), want, "variant 3 (global tables)")
        r.close()
    finally:
        o.close()
        p.close()


# ---- 5. animation: update_instances drops the cache ----------------------------

def test_chain_follows_instance_update():
    o = oracle.OracleScene()
    p = surf_amd.Scene.indoor()
    try:
        ubo = o.camera_ubo(W, H)
        r = surf_amd.Renderer(p, W, H)
        before = r.aov_chain(8)
        assert_planes_equal(before, chain_planes(o, ubo, W, range(H), 8)[0], "before the update")
        o.update(0.5)
        p.update(0.5)
        r.update_instances(p)
        want, _ = chain_planes(o, ubo, W, range(H), 8)
        got = r.aov_chain(8)
        assert_planes_equal(got, want, "after update(0.5)")
        assert any(not np.array_equal(got[name].view(np.uint32), before[name].view(np.uint32)) for name in PLANES)
        r.close()
    finally:
        o.close()
        p.close()


# ---- 6. another max_links recomputes -------------------------------------------

def test_changing_max_links_recomputes(product_scene, chain8, chain2):
    assert not np.array_equal(chain8[0]["id"], chain2[0]["id"])
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert_planes_equal(r.aov_chain(8), chain8[0], "8 links")
        assert_planes_equal(r.aov_chain(2), chain2[0], "then 2 links")
        assert_planes_equal(r.aov_chain(8), chain8[0], "then 8 links again")
    finally:
        r.close()


# ---- 7. row shards -------------------------------------------------------------

def test_chain_row_shards_assemble_to_the_frame(product_scene, chain8):
    specs = [surf_amd.ShardSpec(k, 3, 2) for k in range(3)]          # 19 row blocks, the last a single row
    parts = []
    for s in specs:
        r = surf_amd.Renderer(product_scene, W, H, shard=s)
        parts.append(r.aov_chain(8))
        r.close()
    assert sorted(len(p["id"]) for p in parts) == [12, 12, 13]
    for name in PLANES:
        got = surf_amd.assemble_shards(W, H, [p[name].view(np.float32) for p in parts], specs)
        assert np.array_equal(got.view(np.uint32), chain8[0][name].view(np.uint32)), name


# ---- 8. a read in the middle of a sample stream changes nothing ----------------

def test_chain_read_is_neutral_to_the_sample_stream(product_scene):
    w, h = 32, 24
    out = []
    for read in (True, False):
        r = surf_amd.Renderer(product_scene, w, h)
        r.render(2, 0)
        if read:
            planes = r.aov_chain(8)
            assert (planes["id"][..., 3] >= 1).any()
        r.render(2, 2)
        out.append((r.accumulator(), r.stats()))
        r.close()
    (acc_a, st_a), (acc_b, st_b) = out
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc", "samples"):
        assert st_a[k] == st_b[k], k
    assert st_a["samples"] == 4 * w * h


# ---- 9. the guides switch of the two spatial filters ---------------------------

def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_guides_switch(product_scene, chain8, first_hit):
    chain, first = chain8[0], first_hit[0]
    linked = chain["id"][..., 3] >= 1
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert r.filter_guides() == ("first_hit", 8)
        r.set_sample_squares(True)
        r.render(4, 0)
        acc, sq = r.accumulator(), r.sample_squares()
        tw_first, tw_chain = surf_amd.denoise_image_host(acc, first), surf_amd.denoise_image_host(acc, chain)
        sw_first = surf_amd.denoise_sampled_image_host(acc, sq, first)[0]
        sw_chain = surf_amd.denoise_sampled_image_host(acc, sq, chain)[0]
        assert bits_equal(r.denoise(), tw_first) and bits_equal(r.denoise_sampled(), sw_first)
        # the filters that reproject keep the first-hit planes: their state is reset between the modes
        r.temporal_reset()
        t_first, s_first = r.temporal(), r.svgf()
        r.set_filter_guides("chain", 8)
        assert r.filter_guides() == ("chain", 8)
        got = r.denoise()
        assert bits_equal(got, tw_chain), "surf_denoise with the chain guides is not its host twin on the chain planes"
        assert (got[linked] != tw_first[linked]).any(), "the chain guides change no chain pixel"
        got = r.denoise_sampled()
        assert bits_equal(got, sw_chain), "surf_denoise_sampled with the chain guides is not its host twin on the chain planes"
        assert (got[linked] != sw_first[linked]).any()
        r.temporal_reset()
        assert bits_equal(r.temporal(), t_first) and bits_equal(r.svgf(), s_first)
        r.set_filter_guides("first_hit")
        assert r.filter_guides() == ("first_hit", 8)
        assert bits_equal(r.denoise(), tw_first) and bits_equal(r.denoise_sampled(), sw_first)
    finally:
        r.close()


# ---- 10. status codes and the device-to-device copy ----------------------------

TORCH_COPY = """
import sys
import numpy as np
import torch
import surf_amd
want, w, h = np.load(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
scene = surf_amd.Scene.indoor()
r = surf_amd.Renderer(scene, w, h)
host = r.aov_chain(8)
dev = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda:0")
torch.cuda.synchronize()      # the fill runs on torch's stream, the copy on the renderer's
for k, name in enumerate(surf_amd.AOV_PLANES):
    r.copy_aov_chain_to(k, dev.data_ptr(), 8)
    got = dev.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, host[name].view(np.uint32)), name
    assert np.array_equal(got, want[name]), name
r.close()
scene.close()
print("device copies equal")
"""


def test_chain_status_codes_and_device_copy(chain8, tmp_path):
    lib = surf_amd.load()
    buf = np.zeros((8, 8, 4), np.float32)
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        assert lib.surf_read_aov_chain(h, 0, 8, buf.ctypes.data) == -4         # SURF_ERR_NO_SCENE: nothing uploaded
        assert lib.surf_read_aov_chain(h, 4, 8, buf.ctypes.data) == -1         # SURF_ERR_INVALID: planes are 0..3
        assert lib.surf_read_aov_chain(h, -1, 8, buf.ctypes.data) == -1
        assert lib.surf_read_aov_chain(h, 0, 17, buf.ctypes.data) == -1        # above SURF_AOV_CHAIN_MAX_LINKS
        assert lib.surf_read_aov_chain(h, 0, 8, None) == -1
        assert lib.surf_copy_aov_chain_device(h, 0, 8, None) == -1
        assert lib.surf_copy_aov_chain_device(h, 0, 17, buf.ctypes.data) == -1
        assert lib.surf_set_filter_guides(h, 2, 8) == -1                       # unknown mode
        assert lib.surf_set_filter_guides(h, 1, 17) == -1
        g, n = C.c_int(-1), C.c_uint32(99)
        assert lib.surf_get_filter_guides(h, C.byref(g), C.byref(n)) == 0 and (g.value, n.value) == (0, 8)
        assert lib.surf_set_filter_guides(h, 1, 16) == 0
        assert lib.surf_get_filter_guides(h, C.byref(g), C.byref(n)) == 0 and (g.value, n.value) == (1, 16)
    finally:
        lib.surf_destroy(h)
    # the copy into a torch tensor, in a process of its own: torch has to be imported before the
    # library is loaded, so that both run on one HIP runtime (as bench.py arranges it)
    want = str(tmp_path / "want.npz")
    np.savez(want, **{name: chain8[0][name].view(np.uint32) for name in PLANES})
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([surf_amd.REPO_ROOT, surf_amd._PKG]))
    run = subprocess.run([sys.executable, "-c", TORCH_COPY, want, str(W), str(H)], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "device copies equal" in run.stdout


# ---- 11. the C++ API and the example -------------------------------------------

def test_cpp_example_writes_the_chain_planes(product_scene, tmp_path):
    w, h = 64, 48
    exe = os.path.join(surf_amd._PKG, "build", "render_aov")
    prefix = str(tmp_path / "aov")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(w), str(h), prefix, "8"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = surf_amd.Renderer(product_scene, w, h)
    first, want = r.aov(), r.aov_chain(8)
    r.close()
    assert (want["id"][..., 3] >= 1).sum() >= 20
    for stem, planes in ((prefix, first), (prefix + "_chain", want)):
        raw = np.fromfile(stem + "_planes.bin", np.uint32)
        assert raw.size == 4 * w * h * 4
        raw = raw.reshape(4, h, w, 4)
        for k, name in enumerate(PLANES):
            assert np.array_equal(raw[k], planes[name].view(np.uint32)), (stem, name)
    pfm = read_pfm(prefix + "_chain_normal.pfm")
    assert np.array_equal(np.ascontiguousarray(pfm).view(np.uint32), np.ascontiguousarray(want["normal"][..., :3]).view(np.uint32))
    for name in ("position", "albedo"):
        assert os.path.getsize(f"{prefix}_chain_{name}.pfm") == len(f"PF\n{w} {h}\n-1.0\n") + w * h * 12
