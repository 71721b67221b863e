"""Developer utility: what the per-particle stress and strain read-out costs on the device, next to the render hand-off of the same data.

usage: gpu_fields_prof.py [n_side] [--tree PATH]      (default 100: bench.py's 1 M-particle headline scene)

bench.py's headline scene (neo-Hookean cube on the floor, n_side^3 particles) after 50 substeps. Timed with device events on the data's
own stream, host staging left out: wgs_read_particle_fields_device (64 bytes per particle in 3D) and the yardstick,
wgs_prep_vertex_buffer_device(WGS_RENDER_VOLUME) on the same data — one SVD per particle as well, 96-byte records scattered by particle
id. Median, minimum and maximum of 20 calls after 5 warm-up calls. One JSON line per measurement.

--tree PATH takes the package and its libraries from another checkout (the parent commit's build, for the yardstick as it was before
this entry point existed); a library without wgs_read_particle_fields_device is measured for the yardstick alone."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
tree = ROOT
if "--tree" in args:
    i = args.index("--tree")
    tree = os.path.abspath(args[i + 1])
    del args[i:i + 2]
sys.path.insert(0, tree)
import numpy as np
import torch

from wgsparkl_amd import MpmData, MpmPipeline, scenes

RENDER_VOLUME = 1   # include/wgsparkl_hip.h WGS_RENDER_VOLUME
n_side = int(args[0]) if args else 100
sc = scenes.neo_hookean_cube(n_side=n_side, with_floor=True)
pipe = MpmPipeline(0, 3)
data = MpmData.from_scene(pipe, sc)
pipe.step(data, 50)
data.sync()
stream = torch.cuda.ExternalStream(int(data.device_ptrs().hip_stream))
lib = data.lib


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


def report(what, t, bytes_out):
    print(json.dumps(dict(what=what, tree=os.path.relpath(tree, ROOT), n=int(data.n), median_ms=round(t[0], 4), min_ms=round(t[1], 4),
                          max_ms=round(t[2], 4), ns_per_particle=round(1e6 * t[0] / data.n, 4), bytes_out=int(bytes_out))), flush=True)
    return t[0]


inst = torch.ones(data.n * 24, dtype=torch.float32, device="cuda:0")
torch.cuda.synchronize()
yard = report("prep_vertex_buffer_device(WGS_RENDER_VOLUME), the yardstick",
              timed(lambda: lib.wgs_prep_vertex_buffer_device(data._h, RENDER_VOLUME, C.c_void_p(inst.data_ptr()))), data.n * 96)
if hasattr(lib, "wgs_read_particle_fields_device"):
    words = C.sizeof(data.T.ParticleField) // 4
    out = torch.zeros(data.n * words, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    t = report("particle_fields_device", timed(lambda: data.particle_fields_device(out.data_ptr())), data.n * words * 4)
    rec = out.view(-1, words)
    vm = rec[:, 10].view(torch.float32)
    print(json.dumps(dict(what="ratio particle_fields_device / yardstick (this process)", ratio=round(t / yard, 3), limit=1.25,
                          finite_von_mises=bool(torch.isfinite(vm).all().item()), mean_von_mises=float(vm.mean().item()))), flush=True)
