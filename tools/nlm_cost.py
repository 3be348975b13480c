"""Device time of the non-local-means filter's launches (surf_denoise_nlm) by search and
patch radius, the staged filter kernel against the global one.

    python tools/nlm_cost.py [OUT.jsonl]
    env: SIZES (default "1280x720,1920x1080"), REPS (default 5), FRAMES (default 16),
         RADII (default "1:0,3:1,5:2,7:2,7:3,8:3,10:3")

Per size and per SURF_NLM_LDS = 1, 0 (read when the context is created): FRAMES
one-sample frames with two buckets, then per (r, f) a warm-up call and REPS calls of
denoise_nlm() on the unchanged buckets (surf_debug_nlm_time: halves, prepare, filter).
Where the staged layout does not fit (from r + f = 11) both settings run the global
kernel: "staged_requested" is the setting, not the kernel.
Prints one JSON line per setting (and appends them to OUT.jsonl), medians throughout.
MEASUREMENTS "Non-local means" records the figures."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as f:
            f.write(line + "\n")


size = lambda s: tuple(int(v) for v in s.split("x"))
med = lambda v: round(statistics.median(v), 4)
reps, frames = int(os.environ.get("REPS", 5)), int(os.environ.get("FRAMES", 16))
radii = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("RADII", "1:0,3:1,5:2,7:2,7:3,8:3,10:3").split(",")]

scene = surf_amd.Scene.indoor()
for w, h in [size(s) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]:
    for lds in ("1", "0"):
        os.environ["SURF_NLM_LDS"] = lds
        r = surf_amd.Renderer(scene, w, h)
        r.set_sample_buckets(2)
        r.render(frames, 0)
        r.synchronize()
        for sr, pr in radii:
            r.denoise_nlm(search_radius=sr, patch_radius=pr)
            ms = []
            for _ in range(reps):
                r.denoise_nlm(search_radius=sr, patch_radius=pr)
                ms.append(r.debug_nlm_time())
            halves, prepare, filt = ([m[k] for m in ms] for k in range(3))
            emit({"k_nlm": True, "width": w, "height": h, "frames": frames, "reps": reps, "search_radius": sr, "patch_radius": pr,
                  "staged_requested": lds == "1", "halves_ms": med(halves), "prepare_ms": med(prepare), "filter_ms": med(filt),
                  "filter_min_ms": round(min(filt), 4)})
        r.close()
scene.close()
