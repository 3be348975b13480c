"""What the light-map atlas's stages (surf_atlas_build, surf_atlas_finish, surf_atlas_dilate) cost.

    python tools/atlas_cost.py
    env: SIZE (default "1024x1024"), MARGIN (default 2), REPS (default 3)

Two renderers of the atlas's size on the bundled room, one per work mapping of
the cover kernel (SURF_ATLAS_MAP=1, one wave per (triangle, 8 x 8 tile);
SURF_ATLAS_MAP=0, one lane per triangle; the knob is read when the context is
created), both in profiling mode.  The charts are surf_atlas_grid_charts over
every instance.  Per repetition, for each renderer in turn (so the mappings'
launches interleave and see the same clocks): one build into device planes,
one finish of a synthetic accumulator (4 samples a texel) against the build's
albedo plane, one dilate iteration, all between device buffers (the render
path is not run); surf_debug_atlas_time gives the
device times (HIP events on the context's stream, so each figure includes the
events' own few microseconds; the build's first stage includes, under the tile
mapping, the scan and the readback of the item count).  The first repetition
warms up (allocation, code load) and is dropped.  The yardstick beside them is
one k_aov launch over as many pixels in the same process (the camera is moved
and moved back, which drops the cached planes), read through
surf_debug_aov_time.  One JSON line: median, minimum and maximum per stage and
mapping, the build's wall-clock time per mapping (uploads and allocations
included), the ratios to the yardstick, and whether the two mappings' planes
agree word for word.  MEASUREMENTS "Light-map atlas" records the figures."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

lib = surf_amd.load()
reps = int(os.environ.get("REPS", 3))
W, H = (int(v) for v in os.environ.get("SIZE", "1024x1024").split("x"))
margin = int(os.environ.get("MARGIN", 2))
MAPS = {"tile_map": "1", "triangle_map": "0"}
STAGES = ("setup", "cover", "resolve", "finish", "dilate")


def stats(name, ms):
    return {f"{name}_ms": round(statistics.median(ms), 4), f"{name}_min_ms": round(min(ms), 4), f"{name}_max_ms": round(max(ms), 4)}


scene = surf_amd.Scene.indoor()
charts = surf_amd.atlas_grid_charts(scene.desc().instance_count, W, H, margin)
maps = {}
for name, value in MAPS.items():
    os.environ["SURF_ATLAS_MAP"] = value
    maps[name] = surf_amd.Renderer(scene, W, H)
    maps[name].set_profiling(True)
del os.environ["SURF_ATLAS_MAP"]

npx = W * H


class Hip:
    """Device buffers from the HIP runtime the library is linked against (mapped into this process by load()); the
    renderers above are on device 0, which the library made current."""
    with open("/proc/self/maps") as maps:
        rt = C.CDLL(next(line.split()[-1] for line in maps if "libamdhip64.so" in line))
    rt.hipMalloc.argtypes, rt.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    @classmethod
    def malloc(cls, nbytes):
        p = C.c_void_p()
        assert cls.rt.hipMalloc(C.byref(p), nbytes) == 0
        return p.value

    @classmethod
    def free(cls, p):
        cls.rt.hipFree(p)

    @classmethod
    def to_device(cls, dst, src):
        assert cls.rt.hipMemcpy(dst, src.ctypes.data, src.nbytes, 1) == 0       # host to device

    @classmethod
    def to_host(cls, dst, src):
        assert cls.rt.hipMemcpy(dst.ctypes.data, src, dst.nbytes, 2) == 0       # device to host


hip = Hip
bufs = {name: {k: hip.malloc(npx * (1 if "valid" in k else 16)) for k in ("position", "normal", "albedo", "ids", "acc", "lit", "out", "valid", "out_valid")}
        for name in maps}
ubo = scene.camera(W, H)
moved = np.frombuffer(ubo, np.float32).copy()
moved[0] += 0.25                                 # position.x: another camera, so the next set_camera drops the cached planes
moved = moved.tobytes()
plane = np.zeros((H, W, 4), np.float32)

ms = {name: {s: [] for s in STAGES + ("build", "build_wall")} for name in maps}
aov = []
summary = None
acc = np.random.default_rng(1).uniform(0.0, 8.0, (H, W, 4)).astype(np.float32)      # an accumulator to finish: 4 samples a texel
acc[..., 3] = 4.0
for name in maps:
    hip.to_device(bufs[name]["acc"], acc)
for rep in range(reps + 1):
    for name, r in maps.items():
        b = bufs[name]
        t0 = time.perf_counter()
        summary = r.atlas_build_to(scene, charts, W, H, b["position"], b["normal"], b["albedo"], b["ids"])
        wall = (time.perf_counter() - t0) * 1e3
        t = r.debug_atlas_time()
        assert t["tile_map"] == (name == "tile_map")
        r.atlas_finish_to(W, H, b["acc"], b["albedo"], b["lit"], b["valid"])
        t["finish"] = r.debug_atlas_time()["finish"]
        r.atlas_dilate_to(W, H, b["lit"], b["valid"], 1, b["out"], b["out_valid"])
        t["dilate"] = r.debug_atlas_time()["dilate"]
        if rep:
            for s in STAGES:
                ms[name][s].append(t[s])
            ms[name]["build"].append(t["setup"] + t["cover"] + t["resolve"])
            ms[name]["build_wall"].append(wall)
    r = maps["tile_map"]
    r.set_camera(moved)
    r.set_camera(ubo)
    assert lib.surf_read_aov(r.handle, 0, plane.ctypes.data) == 0
    if rep:
        aov.append(r.debug_aov_time())

planes = {}
for name in maps:
    planes[name] = []
    for k in surf_amd.ATLAS_PLANES:
        a = np.zeros((H, W, 4), np.uint32)
        hip.to_host(a, bufs[name][k])
        planes[name].append(a)
equal = all(np.array_equal(a, b) for a, b in zip(planes["tile_map"], planes["triangle_map"]))

line = {"what": "atlas_cost", "width": W, "height": H, "charts": len(charts), "margin": margin, "reps": reps, "maps_equal": equal, **summary}
line.update(stats("k_aov", aov))
for name in maps:
    for s in ("build", "build_wall") + STAGES:
        line.update(stats(f"{name}_{s}", ms[name][s]))
    line[f"{name}_build_over_k_aov"] = round(line[f"{name}_build_ms"] / line["k_aov_ms"], 3)
line["tile_over_triangle_build"] = round(line["tile_map_build_ms"] / line["triangle_map_build_ms"], 3)
line["tile_over_triangle_cover"] = round(line["tile_map_cover_ms"] / line["triangle_map_cover_ms"], 3)
line["finish_over_k_aov"] = round(line["tile_map_finish_ms"] / line["k_aov_ms"], 3)
line["dilate_over_k_aov"] = round(line["tile_map_dilate_ms"] / line["k_aov_ms"], 3)
print(json.dumps(line), flush=True)

for name, r in maps.items():
    for p in bufs[name].values():
        hip.free(p)
    r.close()
scene.close()
