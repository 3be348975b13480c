"""Cost of the mask from the non-local-means filter's error estimate and of the adaptive loop
on it (surf_mask_from_nlm, surf_render_adaptive_nlm).

    python tools/nlm_adaptive_cost.py
    env: SIZES (default "1280x720,1920x1080"), REPS (default 20), FRAMES (default 16), M (default 2),
         LOOP_SIZE (default "1280x720"; empty: skip), MAX (default 64), BATCH (default 16),
         THRESHOLD, SMOOTH, DILATE (defaults: the library's)

Per size one JSON line:
  mask:  FRAMES one-sample frames with M buckets, then REPS calls of mask_from_nlm(): the device
         times (HIP events) of the mask kernel and the compaction
         (surf_debug_error_mask_time) and of the filter's halves, prepare and filter launches
         (surf_debug_nlm_time), medians; the call's host wall clock beside them.
Then at LOOP_SIZE the loop's definition stepped from here with the same entry points the library's
loop calls, one JSON line per round:
  round: the device times of halves, prepare, filter, mask and compaction, the wall
         clock of mask_from_nlm(), the active count, and the wall clock of the round's render to
         its drained end (the first line: the min_samples frames every pixel gets).
  loop:  the totals, stats.samples, and the wall clock of one render_adaptive_nlm() call of the
         same parameters on a cleared accumulator.
MEASUREMENTS "Error-driven adaptive sampling" records the figures."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402

size = lambda s: tuple(int(v) for v in s.split("x"))
env = lambda k, d: int(os.environ.get(k, d))
sizes = [size(s) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",") if s]
reps, frames, M = env("REPS", 20), env("FRAMES", 16), env("M", 2)
med = lambda v: round(statistics.median(v), 4)
defaults = surf_amd.error_mask_params()
mask = dict(threshold=float(os.environ.get("THRESHOLD", defaults.threshold)), smooth=env("SMOOTH", defaults.smooth),
            dilate=env("DILATE", defaults.dilate))


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


scene = surf_amd.Scene.indoor()
for w, h in sizes:
    r = surf_amd.Renderer(scene, w, h)
    r.set_sample_buckets(M)
    r.render(frames, 0)
    r.synchronize()
    p = dict(min_samples=frames, max_samples=1024, **mask)
    r.mask_from_nlm(**p)
    t_wall, t_mask, t_nlm = [], [], []
    for _ in range(reps):
        t_wall.append(wall(lambda: r.mask_from_nlm(**p)))
        t_mask.append(r.debug_error_mask_time())
        t_nlm.append(r.debug_nlm_time())
    active = r.pixel_mask()[1]
    r.close()
    col = lambda rows, k: med([row[k] for row in rows])
    print(json.dumps({"mask": True, "width": w, "height": h, "frames": frames, "reps": reps, "active": active, **mask,
                      "mask_ms": col(t_mask, 0), "compact_ms": col(t_mask, 1),
                      "halves_ms": col(t_nlm, 0), "prepare_ms": col(t_nlm, 1), "filter_ms": col(t_nlm, 2),
                      "mask_from_nlm_wall_ms": med(t_wall)}), flush=True)

if os.environ.get("LOOP_SIZE", "1280x720"):
    w, h = size(os.environ.get("LOOP_SIZE", "1280x720"))
    mx, batch = env("MAX", 64), env("BATCH", 16)
    p = dict(min_samples=frames, max_samples=mx, **mask)
    r = surf_amd.Renderer(scene, w, h)
    r.set_sample_buckets(M)
    r.render(4, 0)                                                 # warm-up: allocations, graphs
    r.mask_from_nlm(**p)
    r.clear_accumulator()
    before = r.stats()["samples"]
    t_first = wall(lambda: (r.render(frames, 0), r.synchronize()))
    print(json.dumps({"round": 0, "width": w, "height": h, "active": w * h, "frames": frames, "render_wall_ms": round(t_first, 2)}), flush=True)
    f, k, total = frames, 0, {"filter_and_mask_wall_ms": 0.0, "render_wall_ms": t_first}
    while True:
        out = {}
        t_mask = wall(lambda: out.update(active=r.mask_from_nlm(**p)))
        nl, em = r.debug_nlm_time(), r.debug_error_mask_time()
        total["filter_and_mask_wall_ms"] += t_mask
        line = {"round": k + 1, "active": out["active"], "halves_ms": round(nl[0], 4), "prepare_ms": round(nl[1], 4), "filter_ms": round(nl[2], 4),
                "mask_ms": round(em[0], 4), "compact_ms": round(em[1], 4), "mask_from_nlm_wall_ms": round(t_mask, 2)}
        if out["active"] == 0 or f == mx:
            print(json.dumps({**line, "last": True}), flush=True)
            break
        nb = min(batch, mx - f)
        t_render = wall(lambda: (r.render(nb, f), r.synchronize()))
        total["render_wall_ms"] += t_render
        print(json.dumps({**line, "frames": nb, "render_wall_ms": round(t_render, 2)}), flush=True)
        f += nb
        k += 1
    samples = r.stats()["samples"] - before
    r.clear_accumulator()
    res = {}
    t_call = wall(lambda: res.update(r.render_adaptive_nlm(batch=batch, **p)))
    print(json.dumps({"loop": True, "width": w, "height": h, "max_samples": mx, "batch": batch, **mask, "rounds": k, "frames": f, "samples": samples,
                      "mean_samples": round(samples / (w * h), 2), **{a: round(b, 2) for a, b in total.items()},
                      "render_adaptive_nlm": {"wall_ms": round(t_call, 2), "rounds": res["rounds"], "frames": res["frames"], "samples": res["samples"],
                                              "above": res["above"], "max_error": float(res["max_error"])}}), flush=True)
    r.close()
scene.close()
