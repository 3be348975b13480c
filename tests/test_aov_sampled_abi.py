"""The sampled feature buffers' additions to the C-ABI that need no GPU: the
five symbols are declared with their prototypes and exported at an unchanged
ABI version, the default parameters, NULL arguments are returned as status
codes, matte_coverage against a hand-written table, and the Python wrappers'
mode names and checks.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surf_amd

SURF_ERR_INVALID = -1
PROTOTYPES = {
    "surf_aov_sampled_default_params": r"surf_aov_sampled_params\s*\*\s*\w*",
    "surf_read_aov_sampled": r"surf_ctx\s*\*\s*\w*,\s*const\s+surf_aov_sampled_params\s*\*\s*\w*,\s*int\s+\w+,\s*void\s*\*\s*\w*",
    "surf_copy_aov_sampled_device": r"surf_ctx\s*\*\s*\w*,\s*const\s+surf_aov_sampled_params\s*\*\s*\w*,\s*int\s+\w+,\s*void\s*\*\s*\w*",
    "surf_debug_aov_sampled_time": r"surf_ctx\s*\*\s*\w*,\s*float\s*\*\s*\w*",
    "surf_set_filter_guides_sampled": r"surf_ctx\s*\*\s*\w*,\s*const\s+surf_aov_sampled_params\s*\*\s*\w*",
}
HEADER = os.path.join(surf_amd.REPO_ROOT, "include", "surf_hip.h")
MISS = 0xFFFFFFFF


def test_symbols_declared_and_exported_at_abi_4():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = surf_amd.load()
    for name, args in PROTOTYPES.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), code), f"{name} is not declared with its prototype"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+SURF_AOVS_MAX_SAMPLES\s+64\b", code) and re.search(r"#define\s+SURF_GUIDES_SAMPLED\s+2\b", code)
    for k, name in enumerate(("POSITION", "NORMAL", "ALBEDO", "ID", "MATTE_KEY", "MATTE_COUNT", "COUNT")):
        assert re.search(r"\bSURF_AOVS_%s\s*=\s*%d\b" % (name, k), code), name
    assert re.search(r"\bSURF_MATTE_INSTANCE\s*=\s*0\b", code) and re.search(r"\bSURF_MATTE_MATERIAL\s*=\s*1\b", code)
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*surf_aov_sampled_params\s*;", code)
    assert struct and re.findall(r"uint32_t\s+(\w+)\s*;", struct.group(1)) == ["samples", "first_sample", "key", "reserved"]
    assert C.sizeof(surf_amd.AovSampledParams) == 16
    assert [f[0] for f in surf_amd.AovSampledParams._fields_] == ["samples", "first_sample", "key", "reserved"]
    # the existing modes keep their values and names
    assert re.search(r"\bSURF_GUIDES_FIRST_HIT\s*=\s*0\b", code) and re.search(r"\bSURF_GUIDES_CHAIN\s*=\s*1\b", code)
    assert lib.surf_abi_version() == 4


def test_cpp_api_declares_the_sampled_planes():
    text = open(os.path.join(surf_amd.REPO_ROOT, "include", "surf", "surf_host.hpp")).read()
    for name in ("readAOVSampled", "readAOVSampledIds", "setFilterGuidesSampled"):
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_default_params():
    lib = surf_amd.load()
    q = surf_amd.AovSampledParams(9, 9, 9, 9)
    assert lib.surf_aov_sampled_default_params(C.byref(q)) == 0
    assert (q.samples, q.first_sample, q.key, q.reserved) == (16, 0, 0, 0)
    assert lib.surf_aov_sampled_default_params(None) == SURF_ERR_INVALID
    d = surf_amd.aov_sampled_params()
    assert (d.samples, d.first_sample, d.key, d.reserved) == (16, 0, 0, 0)
    m = surf_amd.aov_sampled_params(64, 0xFFFFFFFF, "material")
    assert (m.samples, m.first_sample, m.key, m.reserved) == (64, 0xFFFFFFFF, 1, 0)


def test_null_arguments_are_invalid_not_fatal():
    lib = surf_amd.load()
    buf = np.zeros(64, np.float32)
    ms, q = C.c_float(), surf_amd.aov_sampled_params()
    assert lib.surf_read_aov_sampled(None, C.byref(q), 0, buf.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_copy_aov_sampled_device(None, C.byref(q), 0, buf.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_debug_aov_sampled_time(None, C.byref(ms)) == SURF_ERR_INVALID
    assert lib.surf_set_filter_guides_sampled(None, C.byref(q)) == SURF_ERR_INVALID
    h = C.c_void_p()
    if lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0:      # a context needs a device; the NULL-context calls above do not
        try:
            assert lib.surf_read_aov_sampled(h, None, 0, buf.ctypes.data) == SURF_ERR_INVALID
            assert lib.surf_read_aov_sampled(h, C.byref(q), 0, None) == SURF_ERR_INVALID
            assert lib.surf_copy_aov_sampled_device(h, C.byref(q), 0, None) == SURF_ERR_INVALID
            assert lib.surf_debug_aov_sampled_time(h, None) == SURF_ERR_INVALID
            assert lib.surf_set_filter_guides_sampled(h, None) == SURF_ERR_INVALID
        finally:
            lib.surf_destroy(h)


def test_matte_coverage_against_a_hand_written_table():
    # 1 x 3 pixels, 8 samples: a full pixel; three keys and an empty rank; misses beside one key, its table overflown
    keys = np.array([[[5, MISS, MISS, MISS], [7, 2, MISS, MISS], [MISS, 9, 3, 4]]], np.uint32)
    counts = np.array([[[8, 0, 0, 0], [4, 3, 1, 0], [3, 2, 1, 1]]], np.uint32)
    cov = lambda k: surf_amd.matte_coverage(keys, counts, k, 8)
    assert cov(5).dtype == np.float32 and cov(5).shape == (1, 3)
    assert cov(5).tolist() == [[1.0, 0.0, 0.0]]
    assert cov(7).tolist() == [[0.0, 0.5, 0.0]]
    assert cov(2).tolist() == [[0.0, 0.375, 0.0]]
    assert cov(9).tolist() == [[0.0, 0.0, 0.25]]
    # the miss key: empty ranks count nothing; pixel 1 has one miss sample in rank 2, pixel 2 three in rank 0
    assert cov(MISS).tolist() == [[0.0, 0.125, 0.375]]
    assert cov(11).tolist() == [[0.0, 0.0, 0.0]]
    # what the ranks do not cover (pixel 2: one sample fell past the table or the four ranks)
    assert (8 - counts.sum(axis=2)).tolist() == [[0, 0, 1]]
    with pytest.raises(ValueError):
        surf_amd.matte_coverage(keys[0], counts[0], 5, 8)
    with pytest.raises(ValueError):
        surf_amd.matte_coverage(keys, counts[:, :2], 5, 8)
    with pytest.raises(ValueError):
        surf_amd.matte_coverage(keys, counts, 5, 0)


class NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


def test_python_mode_names_and_checks(monkeypatch):
    assert surf_amd.AOVS_PLANES == ("position", "normal", "albedo", "id", "matte_key", "matte_count")
    assert surf_amd.FILTER_GUIDES == ("first_hit", "chain") and surf_amd.FILTER_GUIDES_SAMPLED == "sampled"
    assert surf_amd.MATTE_KEYS == ("instance", "material") and surf_amd.AOVS_MAX_SAMPLES == 64 and surf_amd.MATTE_MISS == MISS
    r = surf_amd.Renderer.__new__(surf_amd.Renderer)     # no context: the checks come before any use of one
    r._h, r.rows, r.width, r.height = None, np.arange(2), 2, 2
    monkeypatch.setattr(surf_amd, "load", lambda: NoLibrary())
    for bad in (dict(samples=0), dict(samples=65), dict(samples=2.5), dict(first_sample=-1), dict(first_sample=1 << 32), dict(key="object")):
        with pytest.raises(ValueError):
            r.aov_sampled(**bad)
        with pytest.raises(ValueError):
            r.copy_aov_sampled_to(0, 0, **bad)
    with pytest.raises(ValueError):
        r.set_filter_guides("sampled", samples=0)
    with pytest.raises(ValueError):
        r.set_filter_guides("sampled", samples=4, first_sample=-1)
    for name in ("second_hit", "Sampled", ""):
        with pytest.raises(ValueError):
            r.set_filter_guides(name)
    monkeypatch.undo()
    r._h = None                                           # nothing for __del__ to destroy
