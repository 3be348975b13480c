"""Device time of k_temporal (surf_temporal_accumulate) at 1280x720 and 1920x1080,
for a static frame and for a frame with the instance moved.

    python tools/temporal_cost.py
    env: SIZES (default "1280x720,1920x1080"), REPS (default 30), SPP (default 1)

Per size: one frame of SPP samples of the indoor scene and two warm-up calls
(buffer allocation, code load, a first history), then
  static: REPS calls of Renderer.temporal() on the unchanged frame -- every hit
          pixel reprojects onto itself and takes one snapped tap;
  moved:  REPS displayed frames of the loop -- Scene.update(0.05),
          update_instances, clear_accumulator, render(1, k, spp=SPP),
          temporal() -- so instance 3's pixels go through the motion table
          and take up to four taps.
Each call's kernel time is surf_debug_temporal_time's (HIP events around the
launch on the context's stream, so the figure includes the events' own few
microseconds).  Prints one JSON line per size with the medians and spreads,
the bytes the kernel moves per pixel -- four current planes in (64 B), four
images out (out, history and the two guide copies the next frame's taps read,
64 B), and the taps (one per pixel in the static case, 48 B, mostly from
cache) -- and the time those bytes take at the achievable HBM rate
(6.3 TB/s).  MEASUREMENTS "Temporal accumulation" records the figures."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
PLANES_IN, IMAGES_OUT, TAP = 64, 64, 48            # bytes per pixel

sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]
reps, spp = int(os.environ.get("REPS", 30)), int(os.environ.get("SPP", 1))


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


for w, h in sizes:
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, w, h)
    r.render(1, spp=spp)
    r.synchronize()
    r.temporal()
    r.temporal()
    static, moved = [], []
    for _ in range(reps):
        r.temporal()
        static.append(r.debug_temporal_time())
    for k in range(1, reps + 1):
        scene.update(0.05)
        r.update_instances(scene)
        r.clear_accumulator()
        r.render(1, first_frame=k * spp, spp=spp)
        r.temporal()
        moved.append(r.debug_temporal_time())
    r.close()
    scene.close()
    st, mv = summary(static), summary(moved)
    floor_ms = (PLANES_IN + IMAGES_OUT) * w * h / HBM_BYTES_PER_S * 1e3
    floor_taps_ms = (PLANES_IN + IMAGES_OUT + TAP) * w * h / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"width": w, "height": h, "reps": reps, "spp": spp,
                      "static": st, "moved": mv, "bytes_per_pixel": PLANES_IN + IMAGES_OUT, "tap_bytes_per_pixel": TAP,
                      "hbm_floor_ms": round(floor_ms, 4), "hbm_floor_with_taps_ms": round(floor_taps_ms, 4),
                      "static_tb_per_s": round((PLANES_IN + IMAGES_OUT) * w * h / (st["median_ms"] * 1e-3) / 1e12, 3),
                      "static_share_of_hbm": round(floor_ms / st["median_ms"], 3)}), flush=True)
