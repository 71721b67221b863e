#!/usr/bin/env python3
"""Developer utility (GPU): what domain walls cost and what they save, one process, the variants of a scene alternating.

    timeout -k 10 800 python tools/gpu_walls_prof.py [cost] [landed] [motive] [rest] [--json FILE]      (no part named: all four)

cost    us per substep of a 2 M Tait fluid block without a floor and of the C2 cube, without walls and with six walls far from every
        particle (every block rejected: the pure cost of the launch)
landed  the 1 M cube resting on the floor collider, on the collider and a floor wall, and on the floor wall alone
motive  block_in_fluid (600 k particles) and a C3-like Drucker-Prager column (432 k), walls="colliders" against the same container as
        domain walls: us per substep and the event-timed passes
rest    how far above the low plane the lowest particles of a settled column rest (sticky and slip, Tait fluid and neo-Hookean)
us per substep: wall clock over `k` substeps between two wgs_sync, median [min, max] of the repetitions; passes: wgs_read_timings of 50
timestamped substeps (each pass includes one timing mark)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wgsparkl_amd import MpmData, MpmPipeline, scenes  # noqa: E402
from wgsparkl_amd.models import (MODEL_FLUID, MODEL_NEO_HOOKEAN, WALL_SLIP, WALL_STICKY, ElasticCoefficients, FluidCoefficients,  # noqa: E402
                                 ParticlePhase, Wall)
from wgsparkl_amd.solver import ParticleSet, SimulationParams  # noqa: E402

OUT = {}


def us_per_substep(pipe, data, k):
    data.sync()
    t0 = time.perf_counter()
    pipe.step(data, k)
    data.sync()
    return (time.perf_counter() - t0) / k * 1e6


def ab(pipe, tag, variants, warm=100, k=300, reps=7, passes=False):
    """`variants`: name -> (scene, walls); every variant is created once, then timed `reps` times in turn"""
    datas = {name: MpmData.from_scene(pipe, s, walls=w) for name, (s, w) in variants.items()}
    for d in datas.values():
        pipe.step(d, warm)
        d.sync()
    times = {name: [] for name in datas}
    for _ in range(reps):
        for name, d in datas.items():
            times[name].append(us_per_substep(pipe, d, k))
    rec = {name: dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), n=int(datas[name].n)) for name, v in times.items()}
    if passes:
        for name, d in datas.items():
            pipe.step(d, 50, True)
            d.sync()
            rec[name]["pass_us_per_substep"] = {p: round(ms * 1e3 / 50, 2) for p, ms in d.read_timings().items()}
            rec[name]["stats"] = {q: d.stats()[q] for q in ("num_active_blocks", "num_near_collider_blocks")}
    OUT[tag] = rec
    print(tag, json.dumps(rec), flush=True)
    for d in datas.values():
        d.close()


def part_cost(pipe):
    far = [Wall(WALL_SLIP, 0.0, -400 if f % 2 == 0 else 900) for f in range(6)]
    sc = scenes.tait_fluid_block(128, 125, 125, with_floor=False)
    ab(pipe, "launch_cost_tait_fluid_block_2M_no_floor", {"no_walls": (sc, None), "six_walls_far": (sc, far)})
    sc = scenes.config_scene("c2")
    ab(pipe, "launch_cost_c2_cube_1M", {"no_walls": (sc, None), "six_walls_far": (sc, far)}, reps=15)


def part_landed(pipe):
    sc = scenes.neo_hookean_cube(100, with_floor=True)
    sc["particles"].pos[:, 1] -= np.float32(5.6)                      # resting on the floor (top face at y = 2)
    floor = [None, None, Wall(WALL_SLIP, 0.0, 2), None, None, None]
    ab(pipe, "landed_cube_1M", {"floor_collider": (sc, None), "floor_collider_and_floor_wall": (sc, floor), "floor_wall_only": (dict(sc, colliders=[]), floor)},
       warm=300, passes=True)


def part_motive(pipe):
    a = scenes.block_in_fluid(dim=3, tank=(96, 64, 96), block=24)
    b = scenes.block_in_fluid(dim=3, tank=(96, 64, 96), block=24, walls="grid")
    for s in (a, b):
        s["grid_capacity"] = 16384
    ab(pipe, "block_in_fluid_600k", {"colliders": (a, None), "grid": (b, b["walls"])}, warm=300, reps=15, passes=True)
    a = scenes.sand_column(60, 120, 60, with_walls=True)
    a["particles"].pos[:, 1] -= np.float32(5.8)                       # standing on the floor (top face at y = 2)
    wl = [Wall.low(18.5, 1.0), Wall.high(51.5, 1.0), Wall.low(2.0, 1.0), None, Wall.low(18.5, 1.0), Wall.high(51.5, 1.0)]   # the cuboids' faces
    ab(pipe, "c3_like_column_432k", {"colliders": (a, None), "grid": (dict(a, colliders=[]), wl)}, warm=300, reps=15, passes=True)


def part_rest(pipe, substeps=6000):
    """a 16 x 24 x 16-particle column dropped from 0.6 cells above the low plane of axis 1 into a box of walls, `substeps` substeps; the
    lowest particle over the last third, in cells above the plane"""
    h, plane = 1.0, 2
    rest = {}
    for mat in ("tait_fluid", "neo_hookean"):
        for typ, tname in ((WALL_STICKY, "sticky"), (WALL_SLIP, "slip")):
            pos = scenes.lattice((16, 24, 16), (8.25, plane + 0.6, 8.25), h, jitter=0.05)
            material = FluidCoefficients(2.0e5, 0.0) if mat == "tait_fluid" else ElasticCoefficients.from_young_modulus(2.0e5, 0.3)
            ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, material, phase=ParticlePhase(1.0, scenes.FLT_MAX))
            s = dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0 / 1200.0), colliders=[], cell_width=h, grid_capacity=4096,
                     model=MODEL_FLUID if mat == "tait_fluid" else MODEL_NEO_HOOKEAN, fluid_gamma=7.0)
            walls = [Wall(typ, 0.0, 7), Wall(typ, 0.0, 18), Wall(typ, 0.0, plane), None, Wall(typ, 0.0, 7), Wall(typ, 0.0, 18)]
            d = MpmData.from_scene(pipe, s, walls=walls)
            lows = []
            for i in range(substeps // 100):
                pipe.step(d, 100)
                d.sync()
                if i >= substeps // 150:
                    y = d.read_positions()[:, 1].astype(np.float64)
                    lows.append([float(y.min()), float(np.sort(y)[:256].mean())])
            lows = np.array(lows)
            x = d.read_positions().astype(np.float64)
            rest[f"{mat}_{tname}"] = dict(lowest_above_plane_cells_min=float(lows[:, 0].min() / h - plane), lowest_above_plane_cells_last=float(lows[-1, 0] / h - plane),
                                          lowest_256_mean_above_plane_cells=float(lows[-1, 1] / h - plane), max_speed=float(d.diagnostics().max_speed),
                                          side_min_above_low_x_plane_cells=float(x[:, 0].min() / h - 7), side_max_below_high_x_plane_cells=float(18 - x[:, 0].max() / h),
                                          substeps=substeps)
            print(mat, tname, rest[f"{mat}_{tname}"], flush=True)
            d.close()
    OUT["rest_position"] = rest


PARTS = dict(cost=part_cost, landed=part_landed, motive=part_motive, rest=part_rest)

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
