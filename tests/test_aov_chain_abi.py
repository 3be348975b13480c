"""The chain feature buffers' additions to the C-ABI that need no GPU: the new
symbols and constants are declared and exported at an unchanged ABI version,
NULL arguments are returned as status codes, and the Python wrappers refuse a
bad guides name or max_links before the library sees them.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surf_amd

SURF_ERR_INVALID = -1
SYMBOLS = ("surf_read_aov_chain", "surf_copy_aov_chain_device", "surf_debug_aov_chain_time", "surf_set_filter_guides",
           "surf_get_filter_guides")
HEADER = os.path.join(surf_amd.REPO_ROOT, "include", "surf_hip.h")


def test_symbols_declared_and_exported_at_abi_4():
    text = open(HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = surf_amd.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"#define\s+SURF_AOV_CHAIN_MAX_LINKS\s+16\b", code)
    assert re.search(r"\bSURF_GUIDES_FIRST_HIT\s*=\s*0\b", code) and re.search(r"\bSURF_GUIDES_CHAIN\s*=\s*1\b", code)
    assert surf_amd.AOV_CHAIN_MAX_LINKS == 16 and surf_amd.FILTER_GUIDES == ("first_hit", "chain")
    assert lib.surf_abi_version() == 4


def test_cpp_api_declares_the_chain():
    text = open(os.path.join(surf_amd.REPO_ROOT, "include", "surf", "surf_host.hpp")).read()
    for name in ("readAOVChain", "readAOVChainIds", "setFilterGuides"):
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_null_arguments_are_invalid_not_fatal():
    lib = surf_amd.load()
    buf = np.zeros(64, np.float32)
    ms, g, n = C.c_float(), C.c_int(), C.c_uint32()
    assert lib.surf_read_aov_chain(None, 0, 8, buf.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_copy_aov_chain_device(None, 0, 8, buf.ctypes.data) == SURF_ERR_INVALID
    assert lib.surf_debug_aov_chain_time(None, C.byref(ms)) == SURF_ERR_INVALID
    assert lib.surf_set_filter_guides(None, 0, 8) == SURF_ERR_INVALID
    assert lib.surf_get_filter_guides(None, C.byref(g), C.byref(n)) == SURF_ERR_INVALID


class NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library")


def test_python_wrappers_check_before_the_library(monkeypatch):
    r = surf_amd.Renderer.__new__(surf_amd.Renderer)     # no context: the checks come before any use of one
    r._h, r.rows, r.width, r.height = None, np.arange(2), 2, 2
    monkeypatch.setattr(surf_amd, "load", lambda: NoLibrary())
    with pytest.raises(ValueError):
        r.set_filter_guides("second_hit")
    with pytest.raises(ValueError):
        r.set_filter_guides("chain", 17)
    with pytest.raises(ValueError):
        r.set_filter_guides("first_hit", -1)
    with pytest.raises(ValueError):
        r.aov_chain(17)
    with pytest.raises(ValueError):
        r.aov_chain(2.5)
    with pytest.raises(ValueError):
        r.copy_aov_chain_to(0, 0, 17)
    monkeypatch.undo()
    r._h = None                                           # nothing for __del__ to destroy
