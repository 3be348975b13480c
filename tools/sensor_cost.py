"""Cost of a bake under the surfel sensor beside the camera render of the same view
(surf_set_surfel_sensor).

    python tools/sensor_cost.py [OUT.jsonl]
    env: SIZE (default "1280x720"), FRAMES (default 16), REPS (default 3)

One context in profiling mode (every launch timed and waited for, so the per-kernel
times add up to the call; the wall clock of such a run is not a frame rate), one-sample
frames, unbounded paths.  Three workloads, interleaved, REPS times each after a warm-up
round of all three:
  camera   the bundled view through the camera -- the yardstick, same process;
  view     the bake of that view's first-hit planes (Renderer.aov()'s position and normal set
           as the sensor: sky pixels, if any, are invalid texels);
  floor    the bake of a SIZE grid of upward-facing texels on the floor rectangle
           x, z in [-9, 9], y = -1.
Per workload: clear, FRAMES frames, synchronize; surf_get_stats' ms_regen, ms_extend,
ms_shade, ms_connect, ms_tail, ms_sort and ms_total, the rays traced (extension +
shadow) and Mrays/s = rays / ms_total, and each kernel's nanoseconds per ray it handles.
Prints one JSON line per workload (medians over REPS) and one of ratios to the camera
render, and appends them to OUT.jsonl.  MEASUREMENTS "Surfel sensor" records the figures."""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
KERNELS = ("ms_regen", "ms_extend", "ms_shade", "ms_connect", "ms_tail", "ms_sort", "ms_total")


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


def floor_grid(w, h, x0=-9.0, z0=-9.0, x1=9.0, z1=9.0, y=-1.0):
    f = np.float32
    px = f(x0) + ((np.arange(w, dtype=np.float32) + f(0.5)) / f(w)) * (f(x1) - f(x0))
    pz = f(z0) + ((np.arange(h, dtype=np.float32) + f(0.5)) / f(h)) * (f(z1) - f(z0))
    pos, nrm = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    pos[..., 0], pos[..., 1], pos[..., 2] = px[None, :], f(y), pz[:, None]
    nrm[..., 1] = 1.0
    return pos, nrm


w, h = (int(v) for v in os.environ.get("SIZE", "1280x720").split("x"))
frames, reps = int(os.environ.get("FRAMES", 16)), int(os.environ.get("REPS", 3))
if surf_amd.device_count() < 1:
    sys.exit("sensor_cost: no HIP device (a cost is measured on the GPU or not at all)")
scene = surf_amd.Scene.indoor()
r = surf_amd.Renderer(scene, w, h)
r.set_profiling(True)
planes = r.aov()
workloads = {"camera": None, "view": (planes["position"], planes["normal"]), "floor": floor_grid(w, h)}
rows = {name: [] for name in workloads}
for rep in range(reps + 1):                                       # the first round is the warm-up
    for name, sensor in workloads.items():
        if sensor is None:
            r.set_surfel_sensor(None, None)
        else:
            r.set_surfel_sensor(*sensor)
        r.clear_accumulator()
        r.render(frames, 0, 0)
        r.synchronize()
        st = r.stats()
        st["valid"] = r.sensor()[1]
        if rep:
            rows[name].append(st)
r.close()
scene.close()

med = lambda v: statistics.median(v)
summary = {}
for name, sts in rows.items():
    rays = med([s["n_ext"] + s["n_shadow"] for s in sts])
    row = {"workload": name, "width": w, "height": h, "frames": frames, "reps": reps, "profiling": True, "valid_texels": sts[0]["valid"],
           "samples": sts[0]["samples"], "n_ext": sts[0]["n_ext"], "n_shadow": sts[0]["n_shadow"], "iterations": sts[0]["iterations"]}
    for k in KERNELS:
        row[k] = round(med([s[k] for s in sts]), 3)
        row[k + "_values"] = [round(s[k], 3) for s in sts]
    row["mrays_per_s"] = round(rays / row["ms_total"] / 1e3, 2)
    # what each kernel costs per ray it handles: k_extend and k_shade per extension ray of the wavefront phases, k_connect per shadow ray, k_regen per sample
    wf = max(1, sts[0]["n_ext_wavefront"])                        # (the drain traces the rest inside ms_tail)
    row["n_ext_wavefront"] = sts[0]["n_ext_wavefront"]
    row["ns_per_ext_ray_extend"] = round(row["ms_extend"] * 1e6 / wf, 3)
    row["ns_per_ext_ray_shade"] = round(row["ms_shade"] * 1e6 / wf, 3)
    row["ns_per_shadow_ray_connect"] = round(row["ms_connect"] * 1e6 / max(1, sts[0]["n_shadow"]), 3)
    row["ns_per_sample_regen"] = round(row["ms_regen"] * 1e6 / sts[0]["samples"], 3)
    row["ext_rays_per_sample"] = round(sts[0]["n_ext"] / sts[0]["samples"], 3)
    summary[name] = row
    emit(row)
cam = summary["camera"]
for name in ("view", "floor"):
    s = summary[name]
    emit({"ratio_to_camera": name, **{k: round(s[k] / cam[k], 3) if cam[k] else None for k in KERNELS},
          "mrays_per_s": round(s["mrays_per_s"] / cam["mrays_per_s"], 3),
          "ns_per_ext_ray_extend": round(s["ns_per_ext_ray_extend"] / cam["ns_per_ext_ray_extend"], 3),
          "ns_per_ext_ray_shade": round(s["ns_per_ext_ray_shade"] / cam["ns_per_ext_ray_shade"], 3),
          "ns_per_shadow_ray_connect": round(s["ns_per_shadow_ray_connect"] / cam["ns_per_shadow_ray_connect"], 3),
          "ns_per_sample_regen": round(s["ns_per_sample_regen"] / cam["ns_per_sample_regen"], 3),
          "ext_rays_per_sample": round(s["ext_rays_per_sample"] / cam["ext_rays_per_sample"], 3)})
