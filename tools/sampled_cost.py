"""Device time of the sample-variance-guided filter's kernels (surf_denoise_sampled)
at 1280x720 and 1920x1080, beside the variance-guided filter's first frame and the
fixed-sigma filter on the same accumulator, and of k_accumulate with the squares
plane on and off.

    python tools/sampled_cost.py
    env: SIZES (default "1280x720,1920x1080"), REPS (default 30), FRAMES (default 16),
         ACC_SIZE (default "1280x720"), ACC_FRAMES (default 64), ACC_REPS (default 5)

Per size: FRAMES one-sample frames of the indoor scene with the squares on, a
warm-up of each path, then REPS calls of each on the unchanged accumulator:
  sampled: denoise_sampled()                      (surf_debug_sampled_time)
  svgf:    temporal_reset() + svgf(), a first frame (surf_debug_svgf_time)
  fixed:   denoise()                              (surf_debug_denoise_time)
  noise:   noise_estimate() with and without the image, host wall clock of the call
Then at ACC_SIZE, in profiling mode (every launch timed and waited for), ACC_REPS
times each: clear, ACC_FRAMES one-sample frames, surf_get_stats().ms_accum -- with
the squares off and on, interleaved.  Prints one JSON line per size and one for
k_accumulate, medians throughout.  MEASUREMENTS "Sample-variance-guided filter"
records the figures."""
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
sizes = [size(s) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]
reps, frames = int(os.environ.get("REPS", 30)), int(os.environ.get("FRAMES", 16))
med = lambda rows, pick: round(statistics.median(pick(r) for r in rows), 4)

for w, h in sizes:
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, w, h)
    r.set_sample_squares(True)
    r.render(frames, 0)
    r.synchronize()
    r.denoise_sampled(), r.svgf(), r.denoise(), r.noise_estimate()
    sampled, svgf, fixed, noise, noise_only = [], [], [], [], []
    for _ in range(reps):
        r.denoise_sampled()
        sampled.append(r.debug_sampled_time())
    for _ in range(reps):
        r.temporal_reset()
        r.svgf()
        svgf.append(r.debug_svgf_time())
    for _ in range(reps):
        r.denoise()
        fixed.append(r.debug_denoise_time())
    for rows, image in ((noise, True), (noise_only, False)):
        for _ in range(reps):
            t = time.perf_counter()
            r.noise_estimate(image=image)
            rows.append([(time.perf_counter() - t) * 1e3])
    r.close()
    scene.close()
    print(json.dumps({"width": w, "height": h, "reps": reps, "frames": frames,
                      "sampled": {"level0_ms": med(sampled, lambda v: v[0]), "iterations_ms": med(sampled, lambda v: sum(v[1:])),
                                  "per_iteration_ms": [med(sampled, lambda v, k=k: v[k]) for k in range(1, 6)], "total_ms": med(sampled, sum)},
                      "svgf_first_frame": {"temporal_ms": med(svgf, lambda v: v[0]), "variance_ms": med(svgf, lambda v: v[1]),
                                           "iterations_ms": med(svgf, lambda v: sum(v[2:])), "total_ms": med(svgf, sum)},
                      "fixed": {"prepare_ms": med(fixed, lambda v: v[0]), "iterations_ms": med(fixed, lambda v: sum(v[1:])),
                                "total_ms": med(fixed, sum)},
                      "noise_call_wall_ms": {"with_image": med(noise, sum), "summary_only": med(noise_only, sum)}}), flush=True)

w, h = size(os.environ.get("ACC_SIZE", "1280x720"))
acc_frames, acc_reps = int(os.environ.get("ACC_FRAMES", 64)), int(os.environ.get("ACC_REPS", 5))
scene = surf_amd.Scene.indoor()
r = surf_amd.Renderer(scene, w, h)
r.set_profiling(True)
rows = {False: [], True: []}
for _ in range(acc_reps + 1):                                     # the first round is the warm-up
    for on in (False, True):
        r.clear_accumulator()
        r.set_sample_squares(on)
        r.render(acc_frames, 0)
        rows[on].append(r.stats()["ms_accum"])
r.close()
scene.close()
print(json.dumps({"k_accumulate": True, "width": w, "height": h, "frames": acc_frames, "reps": acc_reps,
                  "ms_accum_off": [round(v, 4) for v in rows[False][1:]], "ms_accum_on": [round(v, 4) for v in rows[True][1:]],
                  "median_off": round(statistics.median(rows[False][1:]), 4), "median_on": round(statistics.median(rows[True][1:]), 4)}), flush=True)
