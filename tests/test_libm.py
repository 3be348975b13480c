"""The glibc-exact sinf/cosf/expf the kernels use (csrc/device/surf_math.h)
against this machine's glibc, on a strided sweep of the ranges the path
tracer uses (tools/verify_libm.c does the exhaustive sweep), and through the
library's host build of the same source.

The device half (marked gpu) runs the same source as compiled for gfx950
(Renderer.debug_math: one lane per element) on EXPF_INPUTS and TRIG_INPUTS
and compares it with glibc (oracle.libm) word for word; the CPU half runs the
same arrays through the host build (surf_debug_math_host), so a device mismatch
says which side is wrong.  What the device adds to the host's proof: the
f64 -> f32 conversion of a denormal expf result, expf's early-outs at 88,
0x1.62e42ep6 and -0x1.9fe368p6, its table walk for large ki, and the f64 fma
chain of the trigonometric reduction, all as gfx950 code.  sinf / cosf inputs
with |y| >= 120 are left out (surf_math.h: that branch is an f64 library call
and not bit-exact); NaN inputs are checked with isnan only, the sign of a NaN
being the machine's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import surf_amd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_strided_sweep_matches_glibc(tmp_path):
    exe = tmp_path / "verify_libm"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-x", "c++", "-I", os.path.join(REPO, "surf-path-tracer_amd", "csrc"),
                    os.path.join(REPO, "tools", "verify_libm.c"), "-o", str(exe), "-lm"], check=True)
    out = subprocess.run([str(exe), "211"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout


def test_library_host_build_matches_glibc():
    lib = surf_amd.load()
    libm = C.CDLL("libm.so.6")
    for name in ("sinf", "cosf", "expf"):
        getattr(libm, name).argtypes = [C.c_float]
        getattr(libm, name).restype = C.c_float
    rng = np.random.default_rng(0)
    th = (rng.random(3000, dtype=np.float32) * np.float32(6.2831855)).tolist()
    ex = (-rng.random(3000, dtype=np.float32) * np.float32(60.0)).tolist()
    assert all(lib.surf_ref_sinf(x) == libm.sinf(x) for x in th)
    assert all(lib.surf_ref_cosf(x) == libm.cosf(x) for x in th)
    assert all(lib.surf_ref_expf(x) == libm.expf(x) for x in ex)


# ---- the arrays both halves run -----------------------------------------------------

# e_expf.c's thresholds (results 0 below the first, inf above the second) and s_sinf.c's pi / 4
EXP_UNDERFLOW, EXP_OVERFLOW, PI_4 = float.fromhex("0x1.9fe368p6"), float.fromhex("0x1.62e42ep6"), float.fromhex("0x1.921fb6p-1")


def bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def floats(lo_bits, hi_bits, stride=1):
    """The floats whose words are lo_bits, lo_bits + stride, ... <= hi_bits."""
    return np.arange(lo_bits, hi_bits + 1, stride, dtype=np.uint32).view(np.float32)


def neighbours(x, k=2):
    b = bits(x)
    return np.arange(b - k, b + k + 1, dtype=np.uint32).view(np.float32)


def expf_inputs():
    """Every float in [-104, -87] (2.2 M: results from 1.6e-38 down through the
    denormals to 0, the early-out at -0x1.9fe368p6 inside), a stride-211 sweep of
    [-110, 0], zeros, infinities, denormal and tiny inputs, the neighbours of
    both early-out thresholds, and 88, 88.8, 89 around the overflow."""
    sign = 0x80000000
    special = np.array([0.0, -0.0, -np.inf, np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 1e-30, -1e-30,
                        1e-10, -1e-10, 88.0, 88.8, 89.0, -88.0, -110.0], np.float32)
    return np.concatenate([floats(bits(-87.0), bits(-104.0)), floats(sign, bits(-110.0), 211), special,
                           neighbours(-EXP_UNDERFLOW), neighbours(EXP_OVERFLOW)])


def trig_inputs():
    """The stride-211 sweep of [0, 6.3] (test_strided_sweep_matches_glibc's), every
    float in [6.28, 6.3] (2 pi, the largest theta cosineTry forms, inside), the
    sweep of [-6.3, 0], |y| < 2^-12 with denormals (the y / 1 early-out), and a
    sweep of [6.3, 119.9] (the reduction up to its bound at 120)."""
    sign = 0x80000000
    tiny = floats(0, bits(2.0 ** -12) + 2, 4099)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 2.0 ** -12, -2.0 ** -12, 0.78539816, -0.78539816, 6.2831855, 119.9], np.float32)
    return np.concatenate([floats(0, bits(6.3), 211), floats(bits(6.28), bits(6.3)), floats(sign, sign | bits(6.3), 211), tiny,
                           -tiny, floats(bits(6.3), bits(119.9), 211), neighbours(PI_4), neighbours(-PI_4), special])


NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def glibc():
    """(inputs, glibc's results) per function, computed once."""
    ex, tr = expf_inputs(), trig_inputs()
    assert 2_200_000 < len(ex) < 9_000_000 and 5_000_000 < len(tr) < 12_000_000
    assert np.abs(tr).max() < 120.0 and not np.isnan(ex).any() and not np.isnan(tr).any()
    want = {"expf": (ex, oracle.libm("expf", ex)), "sinf": (tr, oracle.libm("sinf", tr)), "cosf": (tr, oracle.libm("cosf", tr))}
    # the inputs reach what they are there for: denormal and zero results, both early-outs, the overflow
    e = want["expf"][1]
    assert ((e != 0) & (np.abs(e) < 1.17549435e-38)).sum() > 1_000_000 and (e == 0).sum() > 1000 and np.isinf(e).sum() >= 3
    for _, w in want.values():
        w.setflags(write=False)
    return want


def assert_words_equal(got, want, x, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {len(x)} results differ from glibc, first x = {x[bad[0]]!r} "
                           f"(0x{x.view(np.uint32)[bad[0]]:08x}): got {got[bad[0]]!r}, glibc {want[bad[0]]!r}")


def host_map(op, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros((len(x), 2) if op == "sincosf" else len(x), np.float32)
    assert surf_amd.load().surf_debug_math_host(surf_amd.MATH_OPS.index(op), len(x), x.ctypes.data, out.ctypes.data) == 0
    return out


def check_all(run, glibc, side):
    for op in ("expf", "sinf", "cosf"):
        x, want = glibc[op]
        assert_words_equal(run(op, x), want, x, f"{side} {op}")
        assert np.isnan(run(op, NANS)).all(), f"{side} {op} of a NaN"
    x = glibc["sinf"][0]
    sc = run("sincosf", x)
    assert sc.shape == (len(x), 2)
    assert_words_equal(np.ascontiguousarray(sc[:, 0]), glibc["sinf"][1], x, f"{side} sincosf's sine")
    assert_words_equal(np.ascontiguousarray(sc[:, 1]), glibc["cosf"][1], x, f"{side} sincosf's cosine")
    # ... and equals the separate calls of the same side
    assert np.array_equal(sc[:, 0].view(np.uint32), run("sinf", x).view(np.uint32))
    assert np.array_equal(sc[:, 1].view(np.uint32), run("cosf", x).view(np.uint32))
    assert np.isnan(run("sincosf", NANS)).all()


def test_host_build_matches_glibc_on_the_device_inputs(glibc):
    check_all(host_map, glibc, "host build")
    lib = surf_amd.load()
    x = np.zeros(2, np.float32)
    assert lib.surf_debug_math_host(4, 2, x.ctypes.data, x.ctypes.data) == -1 and lib.surf_debug_math_host(0, 2, None, x.ctypes.data) == -1


@pytest.mark.gpu
def test_device_libm_matches_glibc(glibc, product_scene):
    """gExpf, gSinf, gCosf and gSinCosf as compiled for gfx950, one launch per
    function over a few million inputs."""
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    r = surf_amd.Renderer(product_scene, 8, 8)
    try:
        check_all(r.debug_math, glibc, "device")
    finally:
        r.close()
