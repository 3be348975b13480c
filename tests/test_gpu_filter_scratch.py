"""The image-space filters sharing one context's scratch and timers: the image forms
of the fixed-sigma denoiser, the temporal accumulation, the variance-guided filter
(firefly clamp and feedback on), the sample-variance-guided filter and the noise
estimate, interleaved on a context without a scene while the frame size goes up and
down.  Every filter then meets scratch another filter grew and scratch larger than
its frame.

Bar: bit-exact against the CPU twins, and the zero-padding contract of the
surf_debug_*_time readers: the stages that ran finite and >= 0, every entry past
them exactly 0.0.

No frame exceeds 100 x 37.
"""
import ctypes as C
import math

import pytest

import surf_amd
from test_filter_twins_unaligned import assert_outputs_bitequal, filter_frames, twin_calls

pytestmark = pytest.mark.gpu
SIZES = [(33, 9), (100, 37), (5, 3), (33, 9)]
FILTERS = ("denoise", "temporal", "svgf_ext", "denoise_sampled", "noise")
ITERATIONS = 3                                   # twin_calls' choice for every a-trous filter: steps 1 and 2 staged, 4 not
# reader -> (entries asked for, stages a run leaves); the a-trous readers are asked past their arrays' ends
TIMES = {"denoise": ("surf_debug_denoise_time", 10, 1 + ITERATIONS), "temporal": ("surf_debug_temporal_time", 1, 1),
         "svgf_ext": ("surf_debug_svgf_time", 10, 2 + ITERATIONS), "denoise_sampled": ("surf_debug_sampled_time", 10, 1 + ITERATIONS)}


def read_times(lib, ctx, name):
    reader, count, ran = TIMES[name]
    ms = (C.c_float * count)(*([-1.0] * count))
    args = (ctx, ms) if count == 1 else (ctx, ms, count)
    assert getattr(lib, reader)(*args) == 0
    return list(ms), ran


def test_filters_share_scratch_and_timers():
    lib = surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"
    ctx = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(ctx)) == 0
    want = {}
    try:
        for round_, (w, h) in enumerate(SIZES):
            prev, cur = filter_frames(w, h)
            if (w, h) not in want:
                host = twin_calls(prev, cur, 0)
                want[(w, h)] = {name: host[name]() for name in FILTERS}
            device = twin_calls(prev, cur, 0, ctx=ctx)
            for name in FILTERS:
                what = f"round {round_}, {name} at {w} x {h}"
                assert_outputs_bitequal(device[name](), want[(w, h)][name], what)
                if name not in TIMES:
                    continue
                ms, ran = read_times(lib, ctx, name)
                assert all(math.isfinite(v) and v >= 0.0 for v in ms[:ran]), (what, ms)
                assert all(v == 0.0 for v in ms[ran:]), (what, ms)
                if name == "svgf_ext":
                    ff = C.c_float(-1.0)
                    assert lib.surf_debug_firefly_time(ctx, C.byref(ff)) == 0
                    assert math.isfinite(ff.value) and ff.value >= 0.0, (what, ff.value)
    finally:
        lib.surf_destroy(ctx)
