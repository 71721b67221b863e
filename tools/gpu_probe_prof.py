"""Developer utility: what a grid sample and a grid window cost on the device, next to the fused G2P of the same scene.

usage: gpu_probe_prof.py [n_side] [points]      (default 100 and 1000000: bench.py's headline scene, a million probes)

bench.py's headline scene (neo-Hookean cube on the floor, n_side^3 particles) after 50 substeps. Timed with device events on the data's
own stream, host staging left out: wgs_sample_grid_device on `points` uniformly random points inside the body's bounding box and on as many
points of a regular lattice over it, wgs_read_grid_window_device on the window of the same box. Median, minimum and maximum of 20 calls
after 5 warm-up calls. The yardstick is the fused G2P pass of the same data (20 timestamped single-substep steps, the cost of a timing mark
taken off): a probe does a subset of that kernel's per-particle work. One JSON line per measurement."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from helpers import pipeline
from wgsparkl_amd import MpmData, scenes

n_side = int(sys.argv[1]) if len(sys.argv) > 1 else 100
npts = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
sc = scenes.neo_hookean_cube(n_side=n_side, with_floor=True)
h = sc["cell_width"]
pipe = pipeline(3)
data = MpmData.from_scene(pipe, sc, cell_width=h)
pipe.step(data, 50)
data.sync()
pos = data.read_positions()
lo, hi = pos.min(0), pos.max(0)
stream = torch.cuda.ExternalStream(int(data.device_ptrs().hip_stream))
words = C.sizeof(data.T.GridSample) // 4


def timed(call, warm=5, reps=20):
    ms = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        data.sync()
        if i >= warm:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def report(what, n, t, **extra):
    print(json.dumps(dict(what=what, n=int(n), median_ms=round(t[0], 4), min_ms=round(t[1], 4), max_ms=round(t[2], 4),
                          ns_per_item=round(1e6 * t[0] / n, 3), **extra)), flush=True)


rng = np.random.default_rng(0)
side = int(round(npts ** (1.0 / 3.0)))
axes = [np.linspace(lo[k], hi[k], side, dtype=np.float64) for k in range(3)]
sets = dict(random=rng.uniform(lo, hi, (npts, 3)).astype(np.float32),
            lattice=np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).astype(np.float32))
out = torch.zeros(max(len(p) for p in sets.values()) * words, dtype=torch.int32, device="cuda:0")
for name, pts in sets.items():
    dpts = torch.from_numpy(pts).to("cuda:0")
    torch.cuda.synchronize()
    t = timed(lambda: data.sample_grid_device(dpts.data_ptr(), len(pts), out.data_ptr()))
    active = out[:len(pts) * words].view(-1, words)[:, -1]
    report(f"sample_grid_device, {name} points in the body's bounding box", len(pts), t,
           mean_active_nodes=round(float(active.float().mean().item()), 2), bytes_out=len(pts) * words * 4)

wlo = np.floor(lo / h).astype(np.int64) - 1
wdims = np.ceil(hi / h).astype(np.int64) + 2 - wlo
win = torch.zeros(int(np.prod(wdims)) * 4, dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
t = timed(lambda: data.grid_window_device(wlo, wdims, win.data_ptr()))
report(f"grid_window_device, window {tuple(int(x) for x in wdims)} over the same box", int(np.prod(wdims)), t,
       active_blocks=data.stats()["num_active_blocks"], bytes_out=int(np.prod(wdims)) * 16)

# the yardstick: the fused G2P pass of the same data, per substep (timing marks are barrier packets of their own: their cost comes off)
g2p = []
for i in range(25):
    pipe.step(data, 1, True)
    data.sync()
    tm = data.read_timings()
    ov = C.c_float(0)
    pipe.lib.wgs_read_timing_overhead(data._h, C.byref(ov))
    if i >= 5:
        g2p.append(tm["g2p"] + tm["particles_update"] - (2 if tm["particles_update"] > 0 else 1) * ov.value)
t = (float(np.median(g2p)), float(min(g2p)), float(max(g2p)))
report("fused G2P + particle update of one substep (both launches), same data", data.n, t)
