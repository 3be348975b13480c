"""Every CPU twin of an image-space filter (surf_*_image_host, include/surf_hip.h) with
planes that are only 4-byte aligned.  The interface takes `const float*` planes of
16-byte records; float4 is 16-byte aligned on the host, so a twin that reads a
caller's plane through a float4 pointer has undefined behaviour on such a plane.
CPU only.

Bar: bit-exact.  Every input and every output plane of a call starts 4 bytes past a
16-byte boundary; the result must equal, word for word, the result of the same call
on 16-byte-aligned copies.

tests/test_gpu_filter_scratch.py imports the frames and the calls from here.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
import surf_amd
from test_gpu_aov import expected_planes
from test_svgf_host import albedo_of, lum
from test_temporal_host import shifted

F = np.float32
SIZES = [(5, 3), (33, 9)]
TWINS = ("denoise", "temporal", "svgf", "svgf_ext", "firefly", "denoise_sampled", "noise", "adaptive_mask", "error_mask")


@functools.lru_cache(maxsize=None)
def filter_frames(w, h):
    """(previous, current): two frames of the indoor scene's feature planes at w x h, the
    instance moved and the camera shifted between them, each a dict of read-only planes
    -- 'acc' (seeded colour, 2 samples), 'squares' (second moments that leave every
    channel a positive sample variance), 'position', 'normal', 'albedo', 'id' -- with
    'instances' and 'camera'.  The previous frame also carries a 'history' and 'moments'."""
    rng = np.random.default_rng(1000 * w + h)
    osc = oracle.OracleScene()
    try:
        mats = osc.export()["materials"]
        ubo = osc.camera_ubo(w, h)

        def frame(cam):
            planes, _ = expected_planes(osc, cam, w, range(h))
            acc = np.empty((h, w, 4), np.float32)
            acc[..., :3] = rng.uniform(0.0, 8.0, (h, w, 3)).astype(np.float32)
            acc[..., 3] = F(2.0)
            sq = np.empty((h, w, 4), np.float32)
            sq[..., :3] = (acc[..., :3] * acc[..., :3]) * F(0.6)
            sq[..., 3] = (lum(acc) * lum(acc)) * F(0.6)
            f = {"acc": acc, "squares": sq, "position": planes["position"], "normal": planes["normal"], "id": planes["id"],
                 "albedo": albedo_of(planes["id"], mats), "instances": osc.export()["instances"], "camera": cam}
            return f

        prev = frame(ubo)
        prev["history"] = prev["acc"] * F(0.5)                   # (c, n = 1)
        l = lum(prev["history"])
        prev["moments"] = np.stack([l, l * l * F(1.5), np.ones_like(l), np.zeros_like(l)], -1).astype(np.float32)
        osc.update(0.1)
        cur = frame(shifted(ubo, (0.05, 0.02, 0.03)))
    finally:
        osc.close()
    for f in (prev, cur):
        for a in f.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return prev, cur


def placed(a, shift):
    """A writable copy of `a` whose first byte lies `shift` bytes past a 16-byte boundary:
    two records more than needed are allocated and the copy starts inside them."""
    a = np.ascontiguousarray(a)
    raw = np.empty(a.nbytes + 32, np.uint8)
    start = (-raw.ctypes.data) % 16 + shift
    out = raw[start:start + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    assert out.ctypes.data % 16 == shift
    return out


def twin_calls(prev, cur, shift, ctx=None):
    """name -> a function that makes one call and returns its outputs as a list of arrays.
    ctx None: the *_image_host twins; else the *_image forms on that context.  Every
    plane handed over is `placed` at `shift`."""
    lib = surf_amd.load()
    h, w = cur["acc"].shape[:2]
    npx = w * h
    pl = lambda a: placed(a, shift)
    img = lambda: placed(np.zeros((h, w, 4), np.float32), shift)
    ptr = lambda a: a.ctypes.data
    head = () if ctx is None else (ctx,)
    fn = lambda name: getattr(lib, f"surf_{name}_image" + ("_host" if ctx is None else ""))

    def ok(rc, what):
        assert rc == 0, (what, rc, lib.surf_last_error(ctx).decode())

    def instances(f):
        return np.frombuffer(bytes(f["instances"]), np.uint8).copy()

    def temporal_args(with_svgf):
        keep = [pl(cur[k]) for k in ("acc", "position", "normal", "id")] + [instances(cur)]
        n_inst = len(keep[4]) // surf_amd.RECORD_BYTES["instances"]
        keep += [pl(prev[k]) for k in ("history", "position", "normal", "id")] + [instances(prev)]
        cam = surf_amd.CameraUBO.from_buffer_copy(prev["camera"])
        if not with_svgf:
            f = surf_amd.TemporalFrame(*[ptr(a) for a in keep[:5]], n_inst, 0)
            q = surf_amd.TemporalPrev(*[ptr(a) for a in keep[5:10]], n_inst, 0, cam)
        else:
            keep += [pl(cur["albedo"]), pl(prev["moments"])]
            f = surf_amd.SvgfFrame(*[ptr(a) for a in keep[:5]], n_inst, 0, ptr(keep[10]))
            q = surf_amd.SvgfPrev(*[ptr(a) for a in keep[5:10]], n_inst, 0, cam, ptr(keep[11]))
        return f, q, keep

    def denoise():
        a = [pl(cur[k]) for k in ("acc", "position", "normal", "albedo")]
        out = img()
        p = surf_amd.denoise_params(iterations=3)
        ok(fn("denoise")(*head, w, h, *[ptr(x) for x in a], C.byref(p), ptr(out)), "denoise")
        return [out]

    def temporal():
        f, q, _keep = temporal_args(False)
        res = [img(), img()]
        p = surf_amd.temporal_params()
        ok(fn("temporal")(*head, w, h, C.byref(f), C.byref(q), C.byref(p), *[ptr(x) for x in res]), "temporal")
        return res

    def svgf(ext):
        f, q, _keep = temporal_args(True)
        res = [img() for _ in range(4)]
        p, sp = surf_amd.temporal_params(), surf_amd.svgf_params(iterations=3)
        args = (*head, w, h, C.byref(f), C.byref(q), C.byref(p), C.byref(sp))
        if ext:
            x = surf_amd.svgf_ext(firefly_scale=4.0, feedback=True)
            name = "surf_svgf_image_host_ex" if ctx is None else "surf_svgf_image_ex"
            ok(getattr(lib, name)(*args, C.byref(x), *[ptr(a) for a in res]), name)
        else:
            ok(fn("svgf")(*args, *[ptr(a) for a in res]), "svgf")
        return res

    def firefly():
        a, alb, out = pl(cur["acc"]), pl(cur["albedo"]), img()
        ok(fn("firefly")(*head, w, h, ptr(a), ptr(alb), 1, 2.0, ptr(out)), "firefly")
        return [out]

    def denoise_sampled():
        a = [pl(cur[k]) for k in ("acc", "squares", "position", "normal", "albedo")]
        res = [img(), img()]
        sp = surf_amd.svgf_params(iterations=3)
        ok(fn("denoise_sampled")(*head, w, h, *[ptr(x) for x in a], C.byref(sp), *[ptr(x) for x in res]), "denoise_sampled")
        return res

    def noise():
        a, q = pl(cur["acc"]), pl(cur["squares"])
        err = placed(np.zeros(npx, np.float32), shift)
        p, s = surf_amd.noise_params(threshold=0.2), surf_amd.NoiseSummary()
        ok(fn("noise")(*head, npx, ptr(a), ptr(q), C.byref(p), ptr(err), C.byref(s)), "noise")
        return [err, np.array([s.pixels, s.above], np.uint64), np.array([s.max_error], np.float32)]

    def adaptive_mask():
        a, q = pl(cur["acc"]), pl(cur["squares"])
        mask, lst = placed(np.zeros(npx, np.uint8), shift), placed(np.zeros(npx, np.uint32), shift)
        p, n = surf_amd.adaptive_mask_params(threshold=0.2, min_samples=2, max_samples=4), C.c_uint32()
        ok(fn("adaptive_mask")(*head, w, h, ptr(a), ptr(q), C.byref(p), ptr(mask), ptr(lst), C.byref(n)), "adaptive_mask")
        return [mask, lst[:n.value], np.array([n.value], np.uint32)]

    def error_mask():
        a = [pl(cur[k]) for k in ("acc", "squares", "acc")]               # out, err, acc
        mask, lst = placed(np.zeros(npx, np.uint8), shift), placed(np.zeros(npx, np.uint32), shift)
        p, n = surf_amd.error_mask_params(threshold=0.2, min_samples=2, max_samples=4), C.c_uint32()
        ok(fn("error_mask")(*head, w, h, *[ptr(x) for x in a], C.byref(p), ptr(mask), ptr(lst), C.byref(n)), "error_mask")
        return [mask, lst[:n.value], np.array([n.value], np.uint32)]

    return {"denoise": denoise, "temporal": temporal, "svgf": lambda: svgf(False), "svgf_ext": lambda: svgf(True), "firefly": firefly,
            "denoise_sampled": denoise_sampled, "noise": noise, "adaptive_mask": adaptive_mask, "error_mask": error_mask}


def words(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_outputs_bitequal(got, want, what):
    assert len(got) == len(want), what
    for k, (g, e) in enumerate(zip(got, want)):
        assert g.shape == e.shape and g.dtype == e.dtype, (what, k, g.shape, e.shape)
        bad = np.argwhere(words(g) != words(e))
        assert len(bad) == 0, f"{what}: output {k} differs in {len(bad)} words, first at {bad[0]}"


@pytest.mark.parametrize("name", TWINS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_takes_planes_that_are_only_4_byte_aligned(size, name):
    prev, cur = filter_frames(*size)
    want = twin_calls(prev, cur, 0)[name]()
    got = twin_calls(prev, cur, 4)[name]()
    assert any(words(a).any() for a in want), f"{name}: the aligned call wrote nothing"
    assert_outputs_bitequal(got, want, f"{name} at {size[0]} x {size[1]}, planes 4 bytes past a 16-byte boundary")
