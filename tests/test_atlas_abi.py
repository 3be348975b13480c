"""The light-map atlas's additions to the C-ABI that need no GPU: the symbols are declared and exported at an unchanged
ABI version, the two structs' layouts, what the CPU twins and the grid-chart helper refuse, surf_atlas_grid_charts against
a Python restatement, the C++ names and the Python wrappers' checks.  CPU only."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import surf_amd
from test_atlas_host import Case, F, IDENTITY, U, WHITE, instance_records, material_records, quad

SURF_ERR_INVALID = -1
SURF_ERR_LIMIT = -7
SYMBOLS = ("surf_atlas_build", "surf_atlas_build_device", "surf_atlas_build_host", "surf_atlas_grid_charts", "surf_atlas_finish",
           "surf_atlas_finish_device", "surf_atlas_finish_host", "surf_atlas_dilate", "surf_atlas_dilate_device", "surf_atlas_dilate_host",
           "surf_atlas_bake", "surf_debug_atlas_time")
HEADER = os.path.join(surf_amd.REPO_ROOT, "include", "surf_hip.h")


def test_symbols_declared_and_exported_at_abi_4():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = surf_amd.load()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+instance;\s*uint32_t\s+flags;\s*float\s+scale\[2\],\s*offset\[2\];\s*\}\s*surf_atlas_chart;", code)
    assert re.search(r"typedef\s+struct\s*\{\s*uint32_t\s+covered,\s*overlapped,\s*skipped_triangles,\s*triangles;\s*\}\s*surf_atlas_summary;", code)
    assert C.sizeof(surf_amd.AtlasChart) == 24 and C.sizeof(surf_amd.AtlasSummary) == 16
    assert [getattr(surf_amd.AtlasChart, f).offset for f in ("instance", "flags", "scale", "offset")] == [0, 4, 8, 16]
    assert [getattr(surf_amd.AtlasSummary, f).offset for f in ("covered", "overlapped", "skipped_triangles", "triangles")] == [0, 4, 8, 12]
    assert lib.surf_abi_version() == 4
    assert re.search(r"#define\s+SURF_ABI_VERSION\s+4\b", code)


def test_cpp_api_declares_the_atlas():
    text = open(os.path.join(surf_amd.REPO_ROOT, "include", "surf", "surf_host.hpp")).read()
    for name in ("buildAtlas", "finishAtlas", "dilateAtlas"):
        assert re.search(r"\b%s\s*\(" % name, text), name


def code_of(fn, *args, **kw):
    with pytest.raises(surf_amd.SurfError) as e:
        fn(*args, **kw)
    return e.value.code


def test_build_host_refusals():
    case = quad(8, 8)
    d = case.desc()
    ok = [(0, 0, 1.0, 1.0, 0.0, 0.0)]
    assert surf_amd.atlas_build_host(d, ok, 8, 8)["summary"]["covered"] == 64
    for W, H in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        assert code_of(surf_amd.atlas_build_host, d, ok, W, H) == SURF_ERR_INVALID
    assert code_of(surf_amd.atlas_build_host, d, [], 8, 8) == SURF_ERR_INVALID                               # n_charts == 0
    assert code_of(surf_amd.atlas_build_host, d, [(1, 0, 1.0, 1.0, 0.0, 0.0)], 8, 8) == SURF_ERR_INVALID     # instance out of range
    for bad in ((0, 0, float("nan"), 1.0, 0.0, 0.0), (0, 0, 1.0, float("inf"), 0.0, 0.0), (0, 0, 1.0, 1.0, float("-inf"), 0.0),
                (0, 0, 1.0, 1.0, 0.0, float("nan"))):
        assert code_of(surf_amd.atlas_build_host, d, [bad], 8, 8) == SURF_ERR_INVALID
    projective = quad(8, 8)
    projective.inst[0, 8:24].view(F)[3] = 0.1                                                                # row 3 of M is (0.1, 0, 0, 1)
    assert code_of(surf_amd.atlas_build_host, projective.desc(), ok, 8, 8) == SURF_ERR_INVALID
    for member in ("triangles", "tri_ext", "instances", "materials"):
        e = case.desc()
        setattr(e, member, None)
        assert code_of(surf_amd.atlas_build_host, e, ok, 8, 8) == SURF_ERR_INVALID
    lib = surf_amd.load()
    arr, n = surf_amd.atlas_chart_array(ok)
    assert lib.surf_atlas_build_host(None, arr, n, 8, 8, None, None, None, None, None) == SURF_ERR_INVALID
    assert lib.surf_atlas_build(None, C.byref(d), arr, n, 8, 8, None, None, None, None, None) == SURF_ERR_INVALID
    assert lib.surf_atlas_build_host(C.byref(d), arr, n, 8, 8, None, None, None, None, None) == 0             # every plane and the summary may be NULL


def test_build_host_refuses_offsets_out_of_range():
    ok = [(0, 0, 1.0, 1.0, 0.0, 0.0)]
    for word, value in ((0, 2), (0, 0xFFFFFFFF), (3, 1), (3, 0xFFFFFFFF)):                                   # tri_offset, material_offset
        case = quad(8, 8)                                                                                    # 2 triangles, 1 material
        case.inst[0, word] = value
        assert code_of(surf_amd.atlas_build_host, case.desc(), ok, 8, 8) == SURF_ERR_INVALID


def test_build_host_limit_on_the_triangle_total():
    """65,536 charts over a mesh of 65,536 triangles hold 2^32 keys: SURF_ERR_LIMIT, from the checks alone; the first chart
    alone passes them."""
    n = 65536
    tris, ext = np.zeros((n, 16), F), np.zeros((n, 20), F)                                                   # every triangle skipped (zero area)
    case = Case(tris, ext, instance_records([(0, 0, IDENTITY)]), material_records(WHITE), [], 1, 1)
    charts = np.zeros((n, 6), U)
    charts[:, 2:4] = np.array([1.0, 1.0], F).view(U)                                                         # instance 0, flags 0, scale 1, offset 0
    d, lib = case.desc(), surf_amd.load()
    assert lib.surf_atlas_build_host(C.byref(d), charts.ctypes.data, n, 1, 1, None, None, None, None, None) == SURF_ERR_LIMIT
    assert b"2^32" in lib.surf_last_error(None)
    assert lib.surf_atlas_build_host(C.byref(d), charts.ctypes.data, 1, 1, 1, None, None, None, None, None) == 0


def test_finish_and_dilate_host_refusals():
    lib = surf_amd.load()
    a, v = np.zeros((4, 4, 4), F), np.zeros((4, 4), np.uint8)
    o, ov = np.zeros_like(a), np.zeros_like(v)
    p = lambda x: x.ctypes.data
    assert lib.surf_atlas_finish_host(4, 4, p(a), p(a), p(o), p(ov)) == 0
    assert lib.surf_atlas_finish_host(4, 4, None, p(a), p(o), p(ov)) == SURF_ERR_INVALID
    assert lib.surf_atlas_finish_host(0, 4, p(a), p(a), p(o), p(ov)) == SURF_ERR_INVALID
    assert lib.surf_atlas_finish(None, 4, 4, p(a), p(a), p(o), p(ov)) == SURF_ERR_INVALID
    assert lib.surf_atlas_dilate_host(4, 4, p(a), p(v), 64, p(o), p(ov)) == 0
    assert lib.surf_atlas_dilate_host(4, 4, p(a), p(v), 65, p(o), p(ov)) == SURF_ERR_INVALID
    assert lib.surf_atlas_dilate_host(4, 4, p(a), p(v), 1, p(a), p(ov)) == SURF_ERR_INVALID                   # an output is its own input
    assert lib.surf_atlas_dilate_host(4, 16385, p(a), p(v), 1, p(o), p(ov)) == SURF_ERR_INVALID
    assert lib.surf_atlas_dilate(None, 4, 4, p(a), p(v), 1, p(o), p(ov)) == SURF_ERR_INVALID
    assert lib.surf_debug_atlas_time(None, None, 0, None) == SURF_ERR_INVALID


def py_grid_charts(instances, W, H, margin):
    n = len(instances)
    g = 1
    while g * g < n:
        g += 1
    out = []
    for i, inst in enumerate(instances):
        col, row = i % g, i // g
        lo = (col * W // g + margin, row * H // g + margin)
        hi = ((col + 1) * W // g - margin, (row + 1) * H // g - margin)
        out.append((inst, 0, F(hi[0] - lo[0]) / F(W), F(hi[1] - lo[1]) / F(H), F(lo[0]) / F(W), F(lo[1]) / F(H)))
    return out


@pytest.mark.parametrize("instances,W,H,margin", [([0], 32, 24, 0), ([3, 1, 4, 1, 5], 100, 61, 2), (list(range(11)), 1024, 1024, 2),
                                                   (list(range(16)), 64, 64, 1), (list(range(17)), 16384, 999, 3)])
def test_grid_charts_equal_the_restatement(instances, W, H, margin):
    got = surf_amd.atlas_grid_charts(instances, W, H, margin)
    want = py_grid_charts(instances, W, H, margin)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        row = np.array([g.scale[0], g.scale[1], g.offset[0], g.offset[1]], F)
        assert (g.instance, g.flags) == w[:2] and np.array_equal(row.view(np.uint32), np.array(w[2:], F).view(np.uint32))
    if instances == list(range(len(instances))):
        by_count = surf_amd.atlas_grid_charts(len(instances), W, H, margin)                                  # a count: instances 0..n-1
        assert [bytes(a) for a in by_count] == [bytes(b) for b in got]


def test_grid_charts_refusals():
    for args in ((0, 32, 32, 0), (4, 0, 32, 0), (4, 32, 16385, 0), (4, 32, 32, 8), (4, 32, 32, 100)):
        assert code_of(surf_amd.atlas_grid_charts, *args) == SURF_ERR_INVALID
    assert surf_amd.load().surf_atlas_grid_charts(1, None, 8, 8, 0, None) == SURF_ERR_INVALID


def test_python_wrappers_check_shapes_before_the_library():
    a, v = np.zeros((4, 5, 4), F), np.zeros((4, 5), np.uint8)
    with pytest.raises(ValueError):
        surf_amd.atlas_finish_host(a.astype(np.float64), a)
    with pytest.raises(ValueError):
        surf_amd.atlas_finish_host(a, a[:3])
    with pytest.raises(ValueError):
        surf_amd.atlas_dilate_host(a, v.astype(np.int32), 1)
    with pytest.raises(ValueError):
        surf_amd.atlas_dilate_host(a, v[:, :4], 1)
    with pytest.raises(ValueError):
        surf_amd.atlas_dilate_host(a, v, 65)
    with pytest.raises(ValueError):
        surf_amd.atlas_build_host(quad(8, 8).desc(), [(0, 0, 1.0, 1.0, 0.0, 0.0)], -1, 8)
    for name in ("atlas_build", "atlas_build_to", "atlas_finish", "atlas_dilate", "bake_atlas"):
        assert callable(getattr(surf_amd.Renderer, name)), name
