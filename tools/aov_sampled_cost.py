"""What the sampled feature buffers (surf_read_aov_sampled) cost and what they
are worth as filter guides.

    python tools/aov_sampled_cost.py [cost] [worth]        (default: both)
    env: SIZES (default "1280x720,1920x1080"), SAMPLES (default "1,4,16,64"), REPS (default 10),
         WORTH_SIZES (default "100x37,1280x720"), SPPS (default "4,16,64"), REF_SPP (default 2048)

Kernel time ("cost").  Per size, sample count and repetition the camera is set
to a shifted one and back, which drops both caches; then one plane of aov()
and of aov_sampled(samples) is read, each the first read after the drop, and
surf_debug_aov_time / surf_debug_aov_sampled_time give the launch's device
time (HIP events on the context's stream, so each figure includes the events'
own few microseconds).  One JSON line per size and sample count: the medians,
the spread, and the ratio of the sampled launch to samples x the first-hit
kernel's time in the same process.

Guides ("worth").  Per size the bundled view: REF_SPP samples per pixel as the
baseline (sample indices from 4096, disjoint from the frames under test), then
per spp a frame of spp one-sample frames from index 0 through denoise(),
denoise_sampled() and denoise_regress() at their defaults, with the first-hit
guides and with the sampled guides (samples = spp, first_sample = 0).  MAE of
the RGB radiance over the frame and over the edge pixels -- those whose
64-sample instance matte holds two or more keys.  One JSON line per size and spp.
MEASUREMENTS "Sampled feature buffers" records the figures."""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "surf-path-tracer_amd"))
import surf_amd  # noqa: E402


def sizes_of(name, default):
    return [tuple(int(v) for v in s.split("x")) for s in os.environ.get(name, default).split(",")]


parts = [a for a in sys.argv[1:] if a in ("cost", "worth")] or ["cost", "worth"]
lib = surf_amd.load()
scene = surf_amd.Scene.indoor()


def cost():
    reps = int(os.environ.get("REPS", 10))
    counts = [int(v) for v in os.environ.get("SAMPLES", "1,4,16,64").split(",")]
    for w, h in sizes_of("SIZES", "1280x720,1920x1080"):
        r = surf_amd.Renderer(scene, w, h)
        ubo = scene.camera(w, h)
        moved = np.frombuffer(ubo, np.float32).copy()
        moved[0] += 0.25                                 # position.x: another camera, so the next set_camera drops the caches
        moved = moved.tobytes()
        buf = np.zeros((h, w, 4), np.float32)
        for n in counts:
            q = surf_amd.aov_sampled_params(n)
            first, sampled = [], []
            for rep in range(reps + 1):                  # the first repetition warms up (allocation, code load)
                r.set_camera(moved)
                r.set_camera(ubo)
                assert lib.surf_read_aov(r.handle, 0, buf.ctypes.data) == 0
                assert lib.surf_read_aov_sampled(r.handle, C.byref(q), 0, buf.ctypes.data) == 0
                if rep:
                    first.append(r.debug_aov_time())
                    sampled.append(r.debug_aov_sampled_time())
            a, s = statistics.median(first), statistics.median(sampled)
            print(json.dumps({"what": "cost", "width": w, "height": h, "samples": n, "reps": reps,
                              "k_aov_ms": round(a, 4), "k_aov_min_ms": round(min(first), 4), "k_aov_max_ms": round(max(first), 4),
                              "k_aov_sampled_ms": round(s, 4), "k_aov_sampled_min_ms": round(min(sampled), 4),
                              "k_aov_sampled_max_ms": round(max(sampled), 4), "samples_x_k_aov_ms": round(n * a, 4),
                              "ratio_to_samples_x_k_aov": round(s / (n * a), 3)}), flush=True)
        r.close()


def worth():
    ref_spp = int(os.environ.get("REF_SPP", 2048))
    spps = [int(v) for v in os.environ.get("SPPS", "4,16,64").split(",")]
    for w, h in sizes_of("WORTH_SIZES", "100x37,1280x720"):
        ref_r = surf_amd.Renderer(scene, w, h)
        ref_r.render(ref_spp, 4096)
        acc = ref_r.accumulator()
        ref = (acc[..., :3] / acc[..., 3:]).astype(np.float64)
        ref_r.close()
        r = surf_amd.Renderer(scene, w, h)
        r.set_sample_squares(True)                       # denoise_sampled()'s input
        r.set_sample_buckets(4)                          # denoise_regress()'s input
        edge = r.aov_sampled(64)["matte_count"][..., 1] > 0

        def mae(img):
            e = np.abs(img[..., :3].astype(np.float64) - ref)
            return round(float(e.mean()), 6), round(float(e[edge].mean()), 6)

        filters = {"atrous": lambda: r.denoise(), "sampled_variance": lambda: r.denoise_sampled(), "regress": lambda: r.denoise_regress()[0]}
        for spp in spps:
            r.clear_accumulator()
            r.render(spp, 0)
            acc = r.accumulator()
            line = {"what": "worth", "width": w, "height": h, "spp": spp, "ref_spp": ref_spp, "pixels": w * h, "edge_pixels": int(edge.sum())}
            line["mae_all_unfiltered"], line["mae_edge_unfiltered"] = mae(acc / acc[..., 3:])
            for guides in ("first_hit", "sampled"):
                r.set_filter_guides(guides, samples=spp, first_sample=0)
                for name, run in filters.items():
                    line[f"mae_all_{name}_{guides}"], line[f"mae_edge_{name}_{guides}"] = mae(run())
            for name in filters:
                for where in ("all", "edge"):
                    line[f"ratio_{where}_{name}"] = round(line[f"mae_{where}_{name}_sampled"] / line[f"mae_{where}_{name}_first_hit"], 4)
            print(json.dumps(line), flush=True)
        r.close()


if "cost" in parts:
    cost()
if "worth" in parts:
    worth()
scene.close()
