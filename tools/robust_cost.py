"""Cost of the sample buckets in k_accumulate and device time of the robust estimate's
kernel (surf_set_sample_buckets, surf_robust_accumulator).

    python tools/robust_cost.py [OUT.jsonl]
    env: SIZES (default "1280x720,1920x1080"), REPS (default 20), FRAMES (default 32),
         ACC_SIZE (default "1280x720"), ACC_FRAMES (default 64), ACC_REPS (default 3)

At ACC_SIZE, for M = 0, 4, 8, 16 with the squares off and on, interleaved, ACC_REPS
times each after a warm-up round: clear, ACC_FRAMES one-sample frames under the
default frame batch --
  once in profiling mode (every launch timed and waited for): surf_get_stats().ms_accum
  once without: the host wall clock of render() + synchronize()
Then per size and M = 2, 4, 8, 16: FRAMES one-sample frames with the buckets on, a
warm-up, then REPS calls of robust() on the unchanged planes (surf_debug_robust_time),
beside the bytes the kernel moves, (M + 1) * 16 + 17 per pixel.
Prints one JSON line per setting (and appends them to OUT.jsonl), medians throughout.
MEASUREMENTS "Sample buckets" and "Robust estimate" record the figures."""
import json
import os
import statistics
import sys
import time

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

w, h = size(os.environ.get("ACC_SIZE", "1280x720"))
acc_frames, acc_reps = int(os.environ.get("ACC_FRAMES", 64)), int(os.environ.get("ACC_REPS", 3))
settings = [(m, sq) for sq in (False, True) for m in (0, 4, 8, 16)]
scene = surf_amd.Scene.indoor()
for profiling in (True, False):
    r = surf_amd.Renderer(scene, w, h)
    r.set_profiling(profiling)
    rows = {s: [] for s in settings}
    window = None
    for _ in range(acc_reps + 1):                                 # the first round is the warm-up
        for m, sq in settings:
            r.clear_accumulator()
            r.set_sample_squares(sq)
            r.set_sample_buckets(m)
            t = time.perf_counter()
            r.render(acc_frames, 0)
            r.synchronize()
            wall = (time.perf_counter() - t) * 1e3
            st = r.stats()
            window = st["frame_window"]
            rows[m, sq].append(st["ms_accum"] if profiling else wall)
    r.close()
    for m, sq in settings:
        emit({"k_accumulate": True, "width": w, "height": h, "frames": acc_frames, "reps": acc_reps, "frame_window": window,
              "buckets": m, "squares": sq, "what": "ms_accum" if profiling else "render_wall_ms",
              "values": [round(v, 4) for v in rows[m, sq][1:]], "median": med(rows[m, sq][1:])})

reps, frames = int(os.environ.get("REPS", 20)), int(os.environ.get("FRAMES", 32))
for w, h in [size(s) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]:
    r = surf_amd.Renderer(scene, w, h)
    for m in (2, 4, 8, 16):
        r.clear_accumulator()
        r.set_sample_buckets(m)
        r.render(frames, 0)
        r.synchronize()
        _, _, summary = r.robust()
        ms = []
        for _ in range(reps):
            r.robust()
            ms.append(r.debug_robust_time())
        bytes_px = (m + 1) * 16 + 17
        emit({"k_robust": True, "width": w, "height": h, "frames": frames, "reps": reps, "buckets": m, "trimmed": summary["trimmed"],
              "kernel_ms": med(ms), "min_ms": round(min(ms), 4), "bytes_per_pixel": bytes_px,
              "gb_per_s": round(bytes_px * w * h / (statistics.median(ms) * 1e-3) / 1e9, 1)})
    r.close()
scene.close()
