#!/usr/bin/env python3
"""Developer utility (GPU): what the force fields' launch costs, one process, the variants of one scene alternating.

    timeout -k 10 600 python tools/gpu_forces_prof.py [c2] [fluid] [--json FILE]      (no part named: both)

c2      the C2 cube (1 M particles), fluid: a 2 M Tait fluid block without a floor. Per scene, created once each and timed in turn:
        no_fields          the scene as it is: what it launched before
        rejected           one UNIFORM field in a box far from every particle: every block rejected on its key, the pure cost of the launch
        reached            one UNIFORM field everywhere, of zero acceleration: every block reached, every node read, none written
        reached_written    gravity as a UNIFORM field everywhere (the scene's own gravity off): every node read and written
        eight              eight fields everywhere (radial, vortex, drag, uniform; tiny strengths): the longest rule
        walls              six walls far from every particle, no fields (the figure of notes/round_26.md)
        reached_and_walls  `reached` and `walls` together
us per substep: wall clock over `k` substeps between two wgs_sync, median [min, max] of the repetitions; the difference to no_fields of
the same repetition is reported as well (median [min, max])."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wgsparkl_amd import MpmData, MpmPipeline, scenes  # noqa: E402
from wgsparkl_amd.models import WALL_SLIP, ForceField, Wall  # noqa: E402
from wgsparkl_amd.solver import SimulationParams  # noqa: E402

OUT = {}


def us_per_substep(pipe, data, k):
    data.sync()
    t0 = time.perf_counter()
    pipe.step(data, k)
    data.sync()
    return (time.perf_counter() - t0) / k * 1e6


def variants(sc):
    far_box = ForceField.uniform((0.0, -9.81, 0.0)).within_box((-5000.0, -5000.0, -5000.0), (10.0, 10.0, 10.0))
    far_walls = [Wall(WALL_SLIP, 0.0, -400 if f % 2 == 0 else 900) for f in range(6)]
    idle = ForceField.uniform((0.0, 0.0, 0.0))
    g = sc["params"].gravity
    no_g = dict(sc, params=SimulationParams(gravity=(0.0, 0.0, 0.0), dt=sc["params"].dt))
    c = tuple(float(x) for x in sc["particles"].pos.mean(0))
    eight = [ForceField.radial(c, 1e-3, p, 1.0) for p in range(4)] + [ForceField.vortex(c, 1e-3, (0.2, 1.0, 0.1), p, 1.0) for p in (0, 2)] + \
            [ForceField.drag(1e-3), ForceField.uniform((0.0, -1e-3, 0.0))]
    return {"no_fields": (sc, None, None), "rejected": (sc, [far_box], None), "reached": (sc, [idle], None),
            "reached_written": (no_g, [ForceField.uniform(tuple(g))], None), "eight": (sc, eight, None),
            "walls": (sc, None, far_walls), "reached_and_walls": (sc, [idle], far_walls)}


def ab(pipe, tag, sc, warm=100, k=300, reps=9):
    datas = {name: MpmData.from_scene(pipe, s, forces=f, walls=w) for name, (s, f, w) in variants(sc).items()}
    for d in datas.values():
        pipe.step(d, warm)
        d.sync()
    times = {name: [] for name in datas}
    for _ in range(reps):
        for name, d in datas.items():
            times[name].append(us_per_substep(pipe, d, k))
    base = np.array(times["no_fields"])
    rec = {}
    for name, v in times.items():
        diff = np.array(v) - base
        rec[name] = dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), n=int(datas[name].n),
                         over_no_fields_us=dict(median=float(np.median(diff)), min=float(diff.min()), max=float(diff.max())))
    OUT[tag] = rec
    print(tag, json.dumps(rec), flush=True)
    for d in datas.values():
        d.close()


PARTS = dict(c2=lambda pipe: ab(pipe, "c2_cube_1M", scenes.config_scene("c2")),
             fluid=lambda pipe: ab(pipe, "tait_fluid_block_2M_no_floor", scenes.tait_fluid_block(128, 125, 125, with_floor=False)))

if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--json" in args:
        out = args[args.index("--json") + 1]
        del args[args.index("--json"):args.index("--json") + 2]
    if any(a not in PARTS for a in args):
        sys.exit(__doc__)
    pipe = MpmPipeline(0, 3)
    for name in (args or list(PARTS)):
        PARTS[name](pipe)
        if out:
            with open(out, "w") as f:
                json.dump(OUT, f, indent=1)
