"""Device time of the first-order regression filter's launches (surf_denoise_regress) against
the non-local-means filter's (surf_denoise_nlm) at the same search and patch radius, on the
same context in the same run; the staged filter kernel against the global one.

    python tools/regress_cost.py [OUT.jsonl]
    env: SIZES (default "1280x720,1920x1080"), REPS (default 5), FRAMES (default 16),
         RADII (default "5:2,7:3,10:3")

Per size and per SURF_REGRESS_LDS = 1, 0 (read when the context is created; SURF_NLM_LDS
stays at its default): FRAMES one-sample frames with two buckets, then per (r, f) a
warm-up call and REPS calls of denoise_regress() and of denoise_nlm() on the unchanged
buckets (surf_debug_regress_time, surf_debug_nlm_time: halves, prepare, filter).  Every (r, f) in range fits the staged
layout's bound of 160 KiB; "workgroups_per_cu" is how many of them a compute unit holds.
Prints one JSON line per setting (and appends them to OUT.jsonl), medians throughout;
"ratio" is the regression's filter launch over the non-local-means filter's.
MEASUREMENTS "First-order regression" records the figures."""
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


def lds_bytes(r, f):
    """regressLdsBytes (device/regress_kernels.h)"""
    texels = lambda halo: (32 + 2 * halo) * (8 + 2 * halo)
    return 40 * texels(r + f) + 8 * texels(f) + 32 * texels(r)


size = lambda s: tuple(int(v) for v in s.split("x"))
med = lambda v: round(statistics.median(v), 4)
reps, frames = int(os.environ.get("REPS", 5)), int(os.environ.get("FRAMES", 16))
radii = [tuple(int(v) for v in s.split(":")) for s in os.environ.get("RADII", "5:2,7:3,10:3").split(",")]

scene = surf_amd.Scene.indoor()
for w, h in [size(s) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]:
    for lds in ("1", "0"):
        os.environ["SURF_REGRESS_LDS"] = lds
        r = surf_amd.Renderer(scene, w, h)
        r.set_sample_buckets(2)
        r.render(frames, 0)
        r.synchronize()
        for sr, pr in radii:
            sp = dict(search_radius=sr, patch_radius=pr)
            r.denoise_regress(**sp)
            r.denoise_nlm(**sp)
            ms, nl = [], []
            for _ in range(reps):
                r.denoise_regress(**sp)
                ms.append(r.debug_regress_time())
                r.denoise_nlm(**sp)
                nl.append(r.debug_nlm_time())
            halves, prepare, filt = ([m[k] for m in ms] for k in range(3))
            nlm_filt = [m[2] for m in nl]
            emit({"k_regress": True, "width": w, "height": h, "frames": frames, "reps": reps, "search_radius": sr, "patch_radius": pr,
                  "staged": lds == "1", "lds_bytes": lds_bytes(sr, pr), "workgroups_per_cu": min(2, 160 * 1024 // lds_bytes(sr, pr)) if lds == "1" else 2,
                  "halves_ms": med(halves), "prepare_ms": med(prepare), "filter_ms": med(filt), "filter_min_ms": round(min(filt), 4),
                  "nlm_filter_ms": med(nlm_filt), "ratio": round(statistics.median(filt) / statistics.median(nlm_filt), 3)})
        r.close()
scene.close()
