"""Per-kernel device time of the a-trous denoiser (surf_denoise) at 1280x720 and
1920x1080, for the kernel variant the environment selects.

    SURF_DENOISE_LDS=<largest step staged, 0 = never> python tools/denoise_cost.py
    env: SIZES (default "1280x720,1920x1080"), ITERATIONS (default 5), REPS (default 30), SPP (default 4)

Per size: one frame of SPP samples of the indoor scene, a warm-up run (scratch
allocation, code load), then REPS runs of Renderer.denoise(); each run's kernel
times are surf_debug_denoise_time's (HIP events around every launch on the
context's stream, so each figure includes the event's own few microseconds).
Prints one JSON line per size: the median over the runs of k_denoise_prepare,
of each k_atrous iteration and of their sum, and the spread of the sum.
MEASUREMENTS "Denoiser" records the figures."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]
iterations, reps, spp = int(os.environ.get("ITERATIONS", 5)), int(os.environ.get("REPS", 30)), int(os.environ.get("SPP", 4))
scene = surf_amd.Scene.indoor()
for w, h in sizes:
    r = surf_amd.Renderer(scene, w, h)
    r.render(1, spp=spp)
    r.synchronize()
    r.denoise(iterations=iterations)
    runs = []
    for _ in range(reps):
        r.denoise(iterations=iterations)
        runs.append(r.debug_denoise_time()[: iterations + 1])
    r.close()
    med = [statistics.median(run[k] for run in runs) for k in range(iterations + 1)]
    totals = sorted(sum(run) for run in runs)
    print(json.dumps({"width": w, "height": h, "denoise_lds": os.environ.get("SURF_DENOISE_LDS", "default"),
                      "iterations": iterations, "reps": reps, "prepare_ms": round(med[0], 4),
                      "atrous_ms": [round(v, 4) for v in med[1:]], "total_ms": round(statistics.median(totals), 4),
                      "total_min_ms": round(totals[0], 4), "total_max_ms": round(totals[-1], 4),
                      "unique_traffic_floor_ms": round(64.0 * w * h / 6.29e12 * 1e3, 4)}), flush=True)
scene.close()
