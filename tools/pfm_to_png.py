"""Convert a little-endian PFM (as written by oracle/cpu_ref_bench) to a PNG
with the reference's present-pass gamma (sqrt, fs_quad.frag:22-24).

    python tools/pfm_to_png.py IN.pfm OUT.png [--display [key=value ...]]

With --display the picture goes through the display stage's CPU twin instead
(surf_display_image_host: metered exposure, optional bloom, tone curve, sRGB,
dither; the keys are surf_display_params' fields, the rest keep their defaults)
and the meter's result is printed; that needs the built library, the default
conversion does not."""
import os
import sys
import numpy as np
from PIL import Image

def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        scale = float(f.readline())
        data = np.frombuffer(f.read(), dtype="<f4" if scale < 0 else ">f4")
    return np.flipud(data.reshape(h, w, 3))

def display(img, args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "surf-path-tracer_amd"))
    import surf_amd
    params = dict(a.split("=", 1) for a in args)
    rgba = np.ones(img.shape[:2] + (4,), np.float32)
    rgba[..., :3] = img
    words, meter = surf_amd.display_image_host(rgba, **{k: float(v) for k, v in params.items()})
    print(f"counted {meter['counted']}, black {meter['black']}, median bin {meter['median_bin']}, scale {meter['scale']:g}")
    return words.view(np.uint8).reshape(img.shape[:2] + (4,))[..., :3]

if __name__ == "__main__":
    img = read_pfm(sys.argv[1])
    if len(sys.argv) > 3 and sys.argv[3] == "--display":
        Image.fromarray(display(img, sys.argv[4:])).save(sys.argv[2])
    else:
        img = np.sqrt(np.clip(img, 0.0, 1.0))
        Image.fromarray((img * 255.0 + 0.5).astype(np.uint8)).save(sys.argv[2])
