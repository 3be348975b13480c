"""What the ambient-occlusion pass (surf_read_ao) costs, per lane mapping.

    python tools/ao_cost.py
    env: SIZES (default "1280x720"), SAMPLES (default "16"), RADII (default "1.0,4.0"),
         VARIANTS (default "0,3"), REPS (default 15)

Per scene variant and size two renderers, one per lane mapping (SURF_AO_MAP=0,
one lane per pixel; SURF_AO_MAP=1, one lane per ray; the knob is read when the
context is created).  Per sample count, radius and repetition, for each
renderer in turn (so the two mappings' launches interleave and see the same
clocks): the camera is set to a shifted one and back, which drops the caches;
the first-hit planes are read, so that the occlusion read launches k_ao alone;
then one plane of ao() is read and surf_debug_ao_time gives the launch's device
time (HIP events on the context's stream, so each figure includes the events'
own few microseconds).  The first repetition warms up (allocation, code load)
and is dropped.  The yardstick beside them is one surf_read_aov_sampled launch
of the same sample count, read the same way in the same process.  One JSON line
per variant, size, sample count and radius: median, minimum and maximum per
mapping, the ratio of the medians, and each mapping's ratio to the yardstick.
The two planes of the two mappings are compared word for word once per line.
MEASUREMENTS "Ambient occlusion" records the figures."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

lib = surf_amd.load()
reps = int(os.environ.get("REPS", 15))
sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SIZES", "1280x720").split(",")]
counts = [int(v) for v in os.environ.get("SAMPLES", "16").split(",")]
radii = [float(v) for v in os.environ.get("RADII", "1.0,4.0").split(",")]
variants = [int(v) for v in os.environ.get("VARIANTS", "0,3").split(",")]


def stats(name, ms):
    return {f"{name}_ms": round(statistics.median(ms), 4), f"{name}_min_ms": round(min(ms), 4), f"{name}_max_ms": round(max(ms), 4)}


for variant in variants:
    scene = surf_amd.Scene.indoor(variant=variant)
    for w, h in sizes:
        maps = {}
        for m in ("0", "1"):
            os.environ["SURF_AO_MAP"] = m
            maps[m] = surf_amd.Renderer(scene, w, h)
        del os.environ["SURF_AO_MAP"]
        ubo = scene.camera(w, h)
        moved = np.frombuffer(ubo, np.float32).copy()
        moved[0] += 0.25                                 # position.x: another camera, so the next set_camera drops the caches
        moved = moved.tobytes()
        buf = np.zeros((h, w, 4), np.float32)
        for n in counts:
            sq = surf_amd.aov_sampled_params(n)
            for radius in radii:
                q = surf_amd.ao_params(n, radius)
                ms = {"0": [], "1": [], "sampled": []}
                for rep in range(reps + 1):
                    for m, r in maps.items():
                        r.set_camera(moved)
                        r.set_camera(ubo)
                        assert lib.surf_read_aov(r.handle, 0, buf.ctypes.data) == 0
                        assert lib.surf_read_ao(r.handle, C.byref(q), 0, buf.ctypes.data) == 0
                        if rep:
                            ms[m].append(r.debug_ao_time())
                    r = maps["1"]
                    assert lib.surf_read_aov_sampled(r.handle, C.byref(sq), 0, buf.ctypes.data) == 0
                    if rep:
                        ms["sampled"].append(r.debug_aov_sampled_time())
                a, b = maps["0"].ao(n, radius), maps["1"].ao(n, radius)
                equal = all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in surf_amd.AO_PLANES)
                valid = a["bits"][..., 3] == 1
                line = {"what": "ao_cost", "variant": variant, "width": w, "height": h, "samples": n, "radius": radius, "reps": reps,
                        "valid_pixels": int(valid.sum()), "occluded_share": round(1.0 - float(a["bits"][..., 2][valid].sum()) / (n * max(1, int(valid.sum()))), 4),
                        "maps_equal": equal}
                line.update(stats("pixel_map", ms["0"]))
                line.update(stats("ray_map", ms["1"]))
                line.update(stats("k_aov_sampled", ms["sampled"]))
                line["ray_over_pixel"] = round(line["ray_map_ms"] / line["pixel_map_ms"], 3)
                line["pixel_map_over_sampled"] = round(line["pixel_map_ms"] / line["k_aov_sampled_ms"], 3)
                line["ray_map_over_sampled"] = round(line["ray_map_ms"] / line["k_aov_sampled_ms"], 3)
                print(json.dumps(line), flush=True)
        for r in maps.values():
            r.close()
    scene.close()
