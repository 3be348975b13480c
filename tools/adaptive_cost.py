"""Cost and payoff of the per-pixel sample masks and the adaptive loop
(surf_set_pixel_mask, surf_mask_from_noise, surf_render_adaptive).

    python tools/adaptive_cost.py
    env: SIZES (default "1280x720,1920x1080"), REPS (default 20), FRAMES (default 16),
         ACC_FRAMES (default 64), ACC_REPS (default 3), ROUNDS (default 4), BATCH (default 16),
         PAYOFF_SIZE (default "1280x720"; empty: skip), MAX (default 1024), THRESHOLD (default 0.05),
         BATCHES (default "8,16,32,64")

Per size, one JSON line each:
  pieces:     FRAMES one-sample frames with the squares on, then REPS calls each of
              mask_from_noise() (flags + compaction + the count's read-back) and
              noise_estimate(image=False) (k_noise + its summary's read-back): host wall
              clock of calls that end synchronised, medians.
  accumulate: profiling mode (every launch timed by HIP events and waited for), ACC_REPS
              times each: clear, ACC_FRAMES one-sample frames, surf_get_stats().ms_accum --
              unmasked (k_accumulate) and under seeded random masks of 25 %, 50 % and all
              pixels but one (k_accumulate_list), interleaved.
  drain:      under a 50 % mask, ROUNDS rounds of BATCH frames each ended by a drain (what
              the loop does) against the same ROUNDS * BATCH frames in one stream; wall
              clock to the synchronised end, medians of REPS / 4 runs.
Then at PAYOFF_SIZE, for each batch of BATCHES: render_adaptive(threshold, max_samples=MAX)
against a uniform render of the same total camera samples (rounded to whole frames):
wall time, stats.samples, noise.above at the threshold, and the MAE of the per-pixel
mean against a uniform render of 4x the samples from a disjoint sample range.
MEASUREMENTS "Adaptive sampling" records the figures."""
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

size = lambda s: tuple(int(v) for v in s.split("x"))
env = lambda k, d: int(os.environ.get(k, d))
sizes = [size(s) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",") if s]
reps, frames = env("REPS", 20), env("FRAMES", 16)
acc_frames, acc_reps = env("ACC_FRAMES", 64), env("ACC_REPS", 3)
rounds, batch = env("ROUNDS", 4), env("BATCH", 16)
med = lambda v: round(statistics.median(v), 4)


def wall(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def random_mask(h, w, frac, seed=1):
    return (np.random.default_rng(seed).random((h, w)) < frac).astype(np.uint8)


scene = surf_amd.Scene.indoor()
for w, h in sizes:
    r = surf_amd.Renderer(scene, w, h)
    r.set_sample_squares(True)
    r.render(frames, 0)
    r.synchronize()
    p = dict(threshold=0.05, min_samples=frames, max_samples=1024, dilate=1)
    r.mask_from_noise(**p), r.noise_estimate(image=False)
    t_mask = [wall(lambda: r.mask_from_noise(**p)) for _ in range(reps)]
    t_noise = [wall(lambda: r.noise_estimate(image=False)) for _ in range(reps)]
    active = r.pixel_mask()[1]
    r.close()
    print(json.dumps({"pieces": True, "width": w, "height": h, "frames": frames, "reps": reps, "active": active,
                      "mask_from_noise_wall_ms": med(t_mask), "noise_estimate_wall_ms": med(t_noise)}), flush=True)

    r = surf_amd.Renderer(scene, w, h)
    r.set_profiling(True)
    one_out = np.ones((h, w), np.uint8)
    one_out[0, 0] = 0
    masks = {"unmasked": None, "25%": random_mask(h, w, 0.25), "50%": random_mask(h, w, 0.5), "all but one": one_out}
    rows = {k: [] for k in masks}
    for _ in range(acc_reps + 1):                                  # the first round is the warm-up
        for k, m in masks.items():
            r.clear_accumulator()
            r.set_sample_squares(True)
            r.set_pixel_mask(m)
            r.render(acc_frames, 0)
            rows[k].append(r.stats()["ms_accum"])
    r.close()
    print(json.dumps({"accumulate": True, "width": w, "height": h, "frames": acc_frames, "reps": acc_reps,
                      "ms_accum": {k: [round(x, 4) for x in v[1:]] for k, v in rows.items()},
                      "median": {k: med(v[1:]) for k, v in rows.items()}}), flush=True)

    r = surf_amd.Renderer(scene, w, h)
    m = random_mask(h, w, 0.5)
    split, joined = [], []
    for k in range(max(2, reps // 4) + 1):
        def per_round():
            for j in range(rounds):
                r.render(batch, j * batch)
                r.synchronize()                                    # the drain each round of the loop ends with
        r.clear_accumulator()
        r.set_pixel_mask(m)
        split.append(wall(per_round))
        r.clear_accumulator()
        r.set_pixel_mask(m)
        joined.append(wall(lambda: (r.render(rounds * batch, 0), r.synchronize())))
    r.close()
    print(json.dumps({"drain": True, "width": w, "height": h, "rounds": rounds, "batch": batch, "active": int(m.sum()),
                      "rounds_drained_ms": med(split[1:]), "one_stream_ms": med(joined[1:]),
                      "overhead_per_round_ms": round((med(split[1:]) - med(joined[1:])) / rounds, 4)}), flush=True)

if os.environ.get("PAYOFF_SIZE", "1280x720"):
    w, h = size(os.environ.get("PAYOFF_SIZE", "1280x720"))
    mx, thr = env("MAX", 1024), float(os.environ.get("THRESHOLD", 0.05))
    batches = [int(b) for b in os.environ.get("BATCHES", "8,16,32,64").split(",")]
    mean = lambda A: A[..., :3] / np.maximum(A[..., 3:], 1.0)
    r = surf_amd.Renderer(scene, w, h)
    r.set_sample_squares(True)
    r.render(4, 0)                                                 # warm-up: allocations, graphs
    r.synchronize()
    runs, ref = [], None
    for b in batches:
        r.clear_accumulator()
        out = {}
        ms = wall(lambda: out.update(r.render_adaptive(threshold=thr, max_samples=mx, batch=b)))
        a_mean = mean(r.accumulator())
        a_counts = r.accumulator()[..., 3]
        uni = max(1, round(out["samples"] / (w * h)))
        r.clear_accumulator()                                      # (resets the mask)

        def uniform():
            for f0 in range(0, uni, 256):
                r.render(min(256, uni - f0), f0)
            r.synchronize()
        ms_u = wall(uniform)
        u_mean, u_noise, u_samples = mean(r.accumulator()), r.noise_estimate(threshold=thr, image=False)[1], r.stats()["samples"]
        if ref is None:                                            # 4x the samples, a disjoint range
            r.clear_accumulator()
            for f0 in range(0, 4 * uni, 256):
                r.render(min(256, 4 * uni - f0), 100000 + f0)
            ref, ref_frames = mean(r.accumulator()), 4 * uni
        mae = lambda x: round(float(np.abs(x - ref).mean()), 6)
        runs.append({"batch": b, "adaptive": {"wall_ms": round(ms, 1), "samples": out["samples"], "frames": out["frames"], "rounds": out["rounds"],
                                               "above": out["noise"]["above"], "mae": mae(a_mean), "mean_count": round(float(a_counts.mean()), 2),
                                               "count_min_max": [int(a_counts.min()), int(a_counts.max())]},
                     "uniform": {"wall_ms": round(ms_u, 1), "samples": u_samples, "frames": uni, "above": u_noise["above"], "mae": mae(u_mean)}})
        print(json.dumps({"payoff": True, "width": w, "height": h, "threshold": thr, "max_samples": mx, "reference_frames": ref_frames, **runs[-1]}), flush=True)
    r.close()
scene.close()
