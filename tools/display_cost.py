"""Device time of the display stage's launches (surf_display) by parameter set, and the
one-pass pack surf_display_rgba8 as the yardstick.

    python tools/display_cost.py [OUT.jsonl]
    env: SIZES (default "1280x720,1920x1080"), REPS (default 200), WARMUP (default 3), FRAMES (default 2),
         RADII (default "0,4,8,16": bloom_radius, 0 = the defaults without bloom)

Per size: FRAMES one-sample frames, then per bloom radius WARMUP calls and REPS calls of
display() on the unchanged accumulator (surf_debug_display_time: meter, scale, blur, pack;
HIP events on the context's stream).  "call_ms" is the host clock around the whole call,
which ends in a stream synchronise and includes the copy of the words to the host; the
same clock around display_rgba8() (one pointwise kernel and the same copy) is the
yardstick row, taken in the same run; that entry point has no device timer, so the
yardstick is a call time, not a kernel time.  The row "plain_pack" is the stage's own
one-pass pack with the yardstick's arithmetic -- manual exposure, no curve, sqrt, no
dither -- timed with events like the others.  For the kernels that stream, the bytes they must
move over their time: the meter reads 16 B per pixel, the fused pack reads 16 B and writes
4 B.  Prints one JSON line per row (and appends them to OUT.jsonl), medians throughout.
MEASUREMENTS "Display stage" records the figures."""
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


def clocked(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


size = lambda s: tuple(int(v) for v in s.split("x"))
med = lambda v: round(statistics.median(v), 4)
reps, warmup, frames = int(os.environ.get("REPS", 200)), int(os.environ.get("WARMUP", 3)), int(os.environ.get("FRAMES", 2))
radii = [int(v) for v in os.environ.get("RADII", "0,4,8,16").split(",")]

scene = surf_amd.Scene.indoor()
for w, h in [size(s) for s in os.environ.get("SIZES", "1280x720,1920x1080").split(",")]:
    r = surf_amd.Renderer(scene, w, h)
    r.render(frames, 0)
    r.synchronize()
    npx = w * h
    for _ in range(warmup):
        r.display_rgba8()
    yard = [clocked(r.display_rgba8) for _ in range(reps)]
    emit({"surf_display_rgba8": True, "width": w, "height": h, "frames": frames, "reps": reps, "call_ms": med(yard), "call_min_ms": round(min(yard), 4)})
    plain = dict(exposure_mode=0, exposure=0.5, curve=0, transfer=1, dither=0)
    for R, kw in [(0, plain)] + [(R, {}) for R in radii]:
        for _ in range(warmup):
            r.display(bloom_radius=R, **kw)
        ms, call = [], []
        for _ in range(reps):
            call.append(clocked(lambda: r.display(bloom_radius=R, **kw)))
            ms.append(r.debug_display_time())
        meter, scale, blur, pack = ([m[k] for m in ms] for k in range(4))
        row = {"surf_display": True, "plain_pack": bool(kw), "width": w, "height": h, "frames": frames, "reps": reps, "bloom_radius": R,
               "meter_ms": med(meter), "scale_ms": med(scale), "blur_ms": med(blur), "pack_ms": med(pack),
               "kernels_ms": med([sum(m) for m in ms]), "call_ms": med(call), "call_min_ms": round(min(call), 4),
               "meter_tb_s": round(npx * 16 / (statistics.median(meter) * 1e-3) / 1e12, 3)}
        if R == 0:
            row["pack_bytes_per_pixel"] = 20
            row["pack_tb_s"] = round(npx * 20 / (statistics.median(pack) * 1e-3) / 1e12, 3)
        emit(row)
    r.close()
scene.close()
