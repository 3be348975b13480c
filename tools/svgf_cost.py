"""Device time of the variance-guided filter's kernels (surf_svgf_accumulate) at
1280x720 and 1920x1080, beside the fixed-sigma path it is compared against
(surf_temporal_accumulate with the spatial filter).

    python tools/svgf_cost.py [--firefly SCALE] [--feedback]
    --firefly SCALE: the firefly clamp in front (surf_svgf_ext.firefly_scale);
    --feedback: the first filtered iteration stored as the history.  With either,
    short and long run through surf_svgf_accumulate_ex and every summary gains
    firefly_ms, k_firefly's time (surf_debug_firefly_time; 0 without the clamp),
    which total_ms then includes.
    env: SIZES (default "1280x720,1920x1080"), REPS (default 30), SPP (default 1),
         SURF_SVGF_LDS (1: the variance kernel's taps from its staged tile, 0: from
         global memory -- read when the context is created, so one run per setting)

Per size: one frame of SPP samples of the indoor scene, a warm-up of each path,
then REPS calls of each case on the unchanged frame:
  short:  temporal_reset() before every svgf(): every pixel is a first-frame
          pixel and takes the 49-tap spatial estimate;
  long:   svgf() after eight warm-up frames: every hit pixel's moments are
          longer than spatial_below and the variance kernel takes no tap;
  fixed:  temporal(spatial=True), the fixed-sigma filter on the blend.
Kernel times are surf_debug_svgf_time's, surf_debug_temporal_time's and
surf_debug_denoise_time's (HIP events on the context's stream).  Prints one
JSON line per size with the medians: k_temporal, guides + variance, the
iterations' sum, and the totals.  MEASUREMENTS "Variance-guided filter"
records the figures."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument("--firefly", type=float, default=0.0, metavar="SCALE")
ap.add_argument("--feedback", action="store_true")
args = ap.parse_args()
ext = dict(firefly_scale=args.firefly, feedback=args.feedback) if args.firefly or args.feedback else {}

sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]
reps, spp = int(os.environ.get("REPS", 30)), int(os.environ.get("SPP", 1))
med = lambda rows, pick: round(statistics.median(pick(r) for r in rows), 4)


def svgf_summary(rows):
    """rows: k_firefly's time, then surf_debug_svgf_time's eight"""
    out = {"temporal_ms": med(rows, lambda r: r[1]), "variance_ms": med(rows, lambda r: r[2]),
           "iterations_ms": med(rows, lambda r: sum(r[3:])), "total_ms": med(rows, sum)}
    if ext:
        out["firefly_ms"] = med(rows, lambda r: r[0])
    return out


def svgf_times(r):
    return [r.debug_firefly_time() if args.firefly else 0.0] + r.debug_svgf_time()


for w, h in sizes:
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, w, h)
    r.render(1, spp=spp)
    r.synchronize()
    r.svgf(**ext)
    r.temporal(spatial=True)
    short, long, fixed = [], [], []
    for _ in range(reps):
        r.temporal_reset()
        r.svgf(**ext)
        short.append(svgf_times(r))
    for _ in range(8):
        r.svgf(**ext)
    for _ in range(reps):
        r.svgf(**ext)
        long.append(svgf_times(r))
    for _ in range(reps):
        r.temporal(spatial=True)
        fixed.append([r.debug_temporal_time()] + r.debug_denoise_time())
    r.close()
    scene.close()
    print(json.dumps({"width": w, "height": h, "reps": reps, "spp": spp, "variance_staged": os.environ.get("SURF_SVGF_LDS", "1") != "0",
                      "firefly_scale": args.firefly, "feedback": args.feedback,
                      "short": svgf_summary(short), "long": svgf_summary(long),
                      "fixed": {"temporal_ms": med(fixed, lambda r: r[0]), "prepare_ms": med(fixed, lambda r: r[1]),
                                "iterations_ms": med(fixed, lambda r: sum(r[2:])), "total_ms": med(fixed, sum)}}), flush=True)
