"""What the feature buffers through mirrors and glass (surf_read_aov_chain) cost
and what they buy the a-trous denoiser.

    python tools/aov_chain_cost.py
    env: SIZES (default "1280x720,1920x1080"), REPS (default 20), LINKS (default "0,2,8"),
         REF_SPP (default 4096), TRIALS (default 8)

Kernel time.  Per size and per repetition the camera is set to a shifted one
and back, which drops both caches; then one plane of aov() and of
aov_chain(max_links) is read, each the first read after the drop, and
surf_debug_aov_time / surf_debug_aov_chain_time give the launch's device time
(HIP events on the context's stream, so each figure includes the events' own
few microseconds).  One JSON line per size: the medians and the spread.

Filter error.  The bundled view at 100x37: TRIALS frames of 8 spp (1-spp
frames, disjoint sample indices) through Renderer.denoise() with the first-hit
guides and with the chain guides at 8 links, default parameters; the baseline
is REF_SPP further samples per pixel of the same view.  MAE of the RGB radiance
over the whole frame and over the chain pixels (id.w >= 1), per trial and
averaged; the unfiltered frame's beside them.  One JSON line.
MEASUREMENTS "Planes through mirrors and glass" records the figures."""
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

sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]
reps, ref_spp, trials = int(os.environ.get("REPS", 20)), int(os.environ.get("REF_SPP", 4096)), int(os.environ.get("TRIALS", 8))
links = [int(v) for v in os.environ.get("LINKS", "0,2,8").split(",")]
lib = surf_amd.load()
scene = surf_amd.Scene.indoor()


def med(v):
    return round(statistics.median(v), 4)


for w, h in sizes:
    r = surf_amd.Renderer(scene, w, h)
    ubo = scene.camera(w, h)
    moved = np.frombuffer(ubo, np.float32).copy()
    moved[0] += 0.25                                     # position.x: another camera, so the next set_camera drops the caches
    moved = moved.tobytes()
    buf = np.zeros((h, w, 4), np.float32)
    first, chain = [], {n: [] for n in links}
    ids = r.aov_chain(max(links))["id"]
    for rep in range(reps + 1):                          # the first repetition warms up (allocation, code load)
        for n in links:
            r.set_camera(moved)
            r.set_camera(ubo)
            assert lib.surf_read_aov(r.handle, 0, buf.ctypes.data) == 0
            assert lib.surf_read_aov_chain(r.handle, 0, n, C.c_void_p(buf.ctypes.data)) == 0
            if rep:
                first.append(r.debug_aov_time())
                chain[n].append(r.debug_aov_chain_time())
    r.close()
    line = {"width": w, "height": h, "reps": reps, "k_aov_ms": med(first), "k_aov_min_ms": round(min(first), 4),
            "k_aov_max_ms": round(max(first), 4), "chain_pixels": int((ids[..., 3] >= 1).sum()),
            "pixels_at_max_links": int((ids[..., 3] == max(links)).sum())}
    for n in links:
        line[f"k_aov_chain_{n}_ms"] = med(chain[n])
        line[f"k_aov_chain_{n}_min_ms"] = round(min(chain[n]), 4)
        line[f"k_aov_chain_{n}_max_ms"] = round(max(chain[n]), 4)
        line[f"ratio_{n}"] = round(statistics.median(chain[n]) / statistics.median(first), 3)
    print(json.dumps(line), flush=True)

# ---- filter error at 100x37, 8 spp ----
W, H, SPP = 100, 37, 8
r = surf_amd.Renderer(scene, W, H)
linked = r.aov_chain(8)["id"][..., 3] >= 1
r.render(ref_spp, SPP * trials)
acc = r.accumulator()
ref = acc[..., :3] / acc[..., 3:]


def mae(img):
    e = np.abs(img[..., :3].astype(np.float64) - ref)
    return float(e.mean()), float(e[linked].mean())


rows = {"noisy": [], "first_hit": [], "chain": []}
for t in range(trials):
    r.clear_accumulator()
    r.render(SPP, SPP * t)
    acc = r.accumulator()
    rows["noisy"].append(mae(acc / acc[..., 3:]))
    r.set_filter_guides("first_hit")
    rows["first_hit"].append(mae(r.denoise()))
    r.set_filter_guides("chain", 8)
    rows["chain"].append(mae(r.denoise()))
r.close()
scene.close()
line = {"width": W, "height": H, "spp": SPP, "ref_spp": ref_spp, "trials": trials, "chain_pixels": int(linked.sum()), "max_links": 8}
for name, v in rows.items():
    line[f"mae_all_{name}"] = round(statistics.mean(a for a, _ in v), 5)
    line[f"mae_chain_pixels_{name}"] = round(statistics.mean(b for _, b in v), 5)
    line[f"mae_chain_pixels_{name}_trials"] = [round(b, 5) for _, b in v]
print(json.dumps(line), flush=True)
