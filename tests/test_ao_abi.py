"""The ambient-occlusion pass's additions to the C-ABI that need no GPU: the
four symbols are declared with their prototypes and exported at an unchanged
ABI version, the enum values, the struct's layout, the default parameters,
NULL arguments are returned as status codes, the C++ names, and the Python
wrappers' names and checks.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surf_amd

SURF_ERR_INVALID = -1
PROTOTYPES = {
    "surf_ao_default_params": r"surf_ao_params\s*\*\s*\w*",
    "surf_read_ao": r"surf_ctx\s*\*\s*\w*,\s*const\s+surf_ao_params\s*\*\s*\w*,\s*int\s+\w+,\s*void\s*\*\s*\w*",
    "surf_copy_ao_device": r"surf_ctx\s*\*\s*\w*,\s*const\s+surf_ao_params\s*\*\s*\w*,\s*int\s+\w+,\s*void\s*\*\s*\w*",
    "surf_debug_ao_time": r"surf_ctx\s*\*\s*\w*,\s*float\s*\*\s*\w*",
}
HEADER = os.path.join(surf_amd.REPO_ROOT, "include", "surf_hip.h")
FIELDS = ["samples", "first_sample", "radius", "bias", "source", "max_links", "reserved"]


def test_symbols_declared_and_exported_at_abi_4():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = surf_amd.load()
    for name, args in PROTOTYPES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), code), f"{name} is not declared with its prototype"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+SURF_AO_SEED_SALT\s+0x5AD0CC1Du\b", code)
    for k, name in enumerate(("OPENNESS", "BITS", "COUNT")):
        assert re.search(r"\bSURF_AO_%s\s*=\s*%d\b" % (name, k), code), name
    assert re.search(r"\bSURF_AO_FIRST_HIT\s*=\s*0\b", code) and re.search(r"\bSURF_AO_CHAIN\s*=\s*1\b", code)
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*surf_ao_params\s*;", code)
    assert struct
    decl = re.findall(r"(uint32_t|float)\s+(\w+)\s*(\[\s*2\s*\])?\s*;", struct.group(1))
    assert [(t, n, bool(a)) for t, n, a in decl] == [("uint32_t", "samples", False), ("uint32_t", "first_sample", False), ("float", "radius", False),
                                                     ("float", "bias", False), ("uint32_t", "source", False), ("uint32_t", "max_links", False),
                                                     ("uint32_t", "reserved", True)]
    assert C.sizeof(surf_amd.AoParams) == 32
    assert [f[0] for f in surf_amd.AoParams._fields_] == FIELDS
    assert [getattr(surf_amd.AoParams, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24]
    assert lib.surf_abi_version() == 4


def test_cpp_api_declares_the_occlusion_planes():
    text = open(os.path.join(surf_amd.REPO_ROOT, "include", "surf", "surf_host.hpp")).read()
    for name in ("readAO", "readAOBits"):
        assert re.search(r"\b%s\s*\(\s*const\s+surf_ao_params\s*&" % name, text), name


def as_tuple(q):
    return (q.samples, q.first_sample, np.float32(q.radius), np.float32(q.bias), q.source, q.max_links, tuple(q.reserved))


def test_default_params():
    lib = surf_amd.load()
    default = (16, 0, np.float32(1.0), np.float32(1e-5), 0, 8, (0, 0))
    q = surf_amd.AoParams(9, 9, 9.0, 9.0, 9, 9, (C.c_uint32 * 2)(9, 9))
    assert lib.surf_ao_default_params(C.byref(q)) == 0
    assert as_tuple(q) == default
    assert lib.surf_ao_default_params(None) == SURF_ERR_INVALID
    assert as_tuple(surf_amd.ao_params()) == default
    m = surf_amd.ao_params(64, float("inf"), 0xFFFFFFFF, 0.0, "chain", 16)
    assert as_tuple(m) == (64, 0xFFFFFFFF, np.float32(np.inf), np.float32(0.0), 1, 16, (0, 0))


def test_null_arguments_are_invalid_not_fatal():
    lib = surf_amd.load()
    buf = np.zeros(64, np.float32)
    ms, q = C.c_float(), surf_amd.ao_params()
    assert lib.surf_read_ao(None, C.byref(q), 0, buf.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_copy_ao_device(None, C.byref(q), 0, buf.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_debug_ao_time(None, C.byref(ms)) == SURF_ERR_INVALID
    h = C.c_void_p()
    if lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0:      # a context needs a device; the NULL-context calls above do not
        try:
            assert lib.surf_read_ao(h, None, 0, buf.ctypes.data) == SURF_ERR_INVALID
            assert lib.surf_read_ao(h, C.byref(q), 0, None) == SURF_ERR_INVALID
            assert lib.surf_copy_ao_device(h, C.byref(q), 0, None) == SURF_ERR_INVALID
            assert lib.surf_debug_ao_time(h, None) == SURF_ERR_INVALID
        finally:
            lib.surf_destroy(h)


class NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


def test_python_names_and_checks(monkeypatch):
    assert surf_amd.AO_PLANES == ("openness", "bits") and surf_amd.AO_SOURCES == ("first_hit", "chain")
    r = surf_amd.Renderer.__new__(surf_amd.Renderer)     # no context: the checks come before any use of one
    r._h, r.rows, r.width, r.height = None, np.arange(2), 2, 2
    monkeypatch.setattr(surf_amd, "load", lambda: NoLibrary())
    bad_params = (dict(samples=0), dict(samples=3), dict(samples=65), dict(samples=2.5), dict(samples=128), dict(first_sample=-1),
                  dict(first_sample=1 << 32), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(bias=-1e-5),
                  dict(bias=float("nan")), dict(source="second_hit"), dict(source="chain", max_links=17), dict(max_links=-1))
    for bad in bad_params:
        with pytest.raises(ValueError):
            surf_amd.ao_params(**bad)
        with pytest.raises(ValueError):
            r.ao(**bad)
        with pytest.raises(ValueError):
            r.copy_ao_to(0, 0, **bad)
    for samples in (1, 2, 4, 8, 16, 32, 64):
        assert surf_amd.ao_params(samples).samples == samples
    monkeypatch.undo()
    r._h = None                                           # nothing for __del__ to destroy
