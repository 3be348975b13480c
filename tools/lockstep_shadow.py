"""Shadow rays on the lock-step traversal model (tools/lockstep_sim.cpp with
LOCKSTEP_ANY=1): records C3's NEE shadow rays of 40 rows of frame 7 with the
oracle, orders them by each layout of the shadow key (SURF_SH_KEY 0, 1, 2:
shadowKey in csrc/device/wavefront_kernels.h) and prints the model's wave steps,
lanes per step and triangle tests per TLAS instance -- where k_connect's work
goes -- for layout 0, then one line per layout.
usage: python tools/lockstep_shadow.py"""
import os, subprocess, sys, tempfile
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import oracle as O
exe = os.path.join(tempfile.gettempdir(), "lockstep_sim")
subprocess.run(["g++", "-O2", "-std=c++17", "-msse4.1", "-ffp-contract=off", "-fopenmp", "-I" + os.path.join(REPO, "oracle"),
                os.path.join(REPO, "tools", "lockstep_sim.cpp"), "-o", exe, "-lz"], check=True)
O.load()
S = O.OracleScene()
W = 1280
_, (so, sd, st) = S.record_rays(W, 720, 7, 300 * W, 340 * W, max_ext=1 << 21, max_shadow=1 << 21)
n = len(so)
end = so + sd * st[:, None]
light = (end[:, 0] > 0).astype(np.int64)
lo, hi = so.min(0), so.max(0)
cell = (((so - lo) / (hi - lo + 1e-6)) * 2).astype(np.int64).clip(0, 1)
base = light * 8 + cell[:, 0] * 4 + cell[:, 1] * 2 + cell[:, 2]
d = tempfile.mkdtemp()
env = dict(os.environ, SURF_ASSETS=os.path.join(REPO, "assets"), LOCKSTEP_ANY="1")


def write(order, fn):
    with open(fn, "wb") as f:
        np.array([n], np.uint32).tofile(f)
        np.concatenate([so[order], sd[order], st[order, None]], axis=1).astype(np.float32).tofile(f)


# the heavy instances' world boxes met within the segment [0, tmax): TLAS instances 3, 4, 5 of C3, heaviest first
pos = np.arange(n)
write(pos, os.path.join(d, "raw.bin"))
subprocess.run([exe, os.path.join(d, "raw.bin"), "mask", os.path.join(d, "mask.bin")], check=True, env=env)
heavy = ((np.fromfile(os.path.join(d, "mask.bin"), dtype=np.uint32) >> 3) & 7).astype(np.int64)
many = (heavy & (heavy - 1)) != 0
cls = np.where(many, 0, np.where(heavy & 1, 1, 2))
quad = light * 4 + cell[:, 0] + 2 * cell[:, 2]
keys = {
    0: base,
    1: np.where(heavy != 0, base, 16 + base),
    2: np.where(heavy != 0, cls * 8 + quad, 24 + base),
}
print("shadow rays", n)
print("segments that meet a heavy box: %.1f %% (%s)" % (100.0 * (heavy != 0).mean(),
      ", ".join("%.1f %%" % (100.0 * ((heavy >> h) & 1).mean()) for h in range(3))))
for k, key in keys.items():
    order = np.argsort(key * n + pos, kind="stable")
    fn = os.path.join(d, "sh%d.bin" % k)
    write(order, fn)
    out = subprocess.run([exe, fn], capture_output=True, text=True, check=True, env=env).stdout
    if k == 0:
        print(out)
    print("SURF_SH_KEY=%d (%d bins) | %s" % (k, (16, 32, 40)[k], [l for l in out.splitlines() if l.startswith("groups")][0]), flush=True)
