#!/usr/bin/env python3
"""Developer utility (GPU): what adding particles at run time costs, one process, the variants of one scene alternating.

    timeout -k 10 600 python tools/gpu_emit_prof.py [c2] [fluid] [--json FILE]      (no part named: both)

c2      the C2 cube (1 M particles), fluid: a 2 M Tait fluid block without a floor. Per scene, created once each and timed in turn:
        plain           the scene as it is: what it launched before
        reserved        the same with a particle capacity of 2 x its particles and nothing added: what a reservation costs
        rebuild_every   the same created under WGS_REHASH_PERIOD=1: every substep rebuilds the block table, nothing is emitted
        emitting        one emitter of 4 x 1 x 4 particles above the body, falling at 1/16 cell per substep, a new layer every 8 substeps
                        (`Emitter.nozzle`: the layers do not pile up in a cell): one substep in 8 emits and rebuilds; the particle count
                        grows by less than 1 % over the whole run
us per substep: wall clock over `k` substeps between two wgs_sync, median [min, max] of the repetitions; the difference to `plain` of
the same repetition is reported as well (median [min, max]) — for `emitting`, 8 times that difference is the cost of an emitting substep
(emission + rebuild) over an ordinary one (`per_emitting_substep_us`); for rebuild_every the difference is a rebuild's cost by itself.
(An emitter that keeps putting particles into the SAME cells — a zero velocity and period 1 — is no measurement of the emission: the
rebuild walks a cell's particles as one list, and thousands in one cell cost hundreds of milliseconds per substep.)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wgsparkl_amd import MpmData, MpmPipeline, scenes  # noqa: E402
from wgsparkl_amd.models import Emitter  # noqa: E402
from wgsparkl_amd.solver import ParticleSet  # noqa: E402

OUT = {}
WARM, K, REPS, PERIOD = 100, 200, 9, 8


def us_per_substep(pipe, data, k):
    data.sync()
    t0 = time.perf_counter()
    pipe.step(data, k)
    data.sync()
    return (time.perf_counter() - t0) / k * 1e6


def one_particle(ps):
    return ParticleSet(**{k: (v[:1].copy() if isinstance(v, np.ndarray) else v) for k, v in ps.__dict__.items()})


def make(pipe, sc, name):
    ps = sc["particles"]
    if name == "plain":
        return MpmData.from_scene(pipe, sc)
    if name == "reserved":
        return MpmData.from_scene(pipe, sc, particle_capacity=2 * ps.n)
    if name == "rebuild_every":
        os.environ["WGS_REHASH_PERIOD"] = "1"      # (read once, at creation)
        try:
            return MpmData.from_scene(pipe, sc)
        finally:
            del os.environ["WGS_REHASH_PERIOD"]
    h = sc["cell_width"]
    top = ps.pos.max(0)
    lo = tuple(float(x) for x in (ps.pos.mean(0)[0], top[1] + 2.0 * h, ps.pos.mean(0)[2]))
    proto = one_particle(ps)                       # (the scene's own material: the uniform layouts hold it)
    proto.vel[:] = 0.0
    proto.vel[0, 1] = -h / 16.0 / sc["params"].dt
    em = Emitter.nozzle(proto, lo, (4, 1, 4), h / 2.0, sc["params"].dt, jitter=0.1, seed=1)
    assert em.period == PERIOD
    return MpmData.from_scene(pipe, sc, particle_capacity=ps.n + 16 * ((WARM + K * REPS) // PERIOD + 2), emitters=[em])


def ab(pipe, tag, sc):
    datas = {name: make(pipe, sc, name) for name in ("plain", "reserved", "rebuild_every", "emitting")}
    for d in datas.values():
        pipe.step(d, WARM)
        d.sync()
    times = {name: [] for name in datas}
    for _ in range(REPS):
        for name, d in datas.items():
            times[name].append(us_per_substep(pipe, d, K))
    base = np.array(times["plain"])
    rec = {}
    for name, v in times.items():
        diff = np.array(v) - base
        st = datas[name].stats()
        rec[name] = dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), n=int(datas[name].n),
                         table_rebuilds=int(st["table_rebuilds"]), device_bytes=int(st["device_bytes"]),
                         over_plain_us=dict(median=float(np.median(diff)), min=float(diff.min()), max=float(diff.max())))
    rec["emitting"]["per_emitting_substep_us"] = {k: PERIOD * v for k, v in rec["emitting"]["over_plain_us"].items()}
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
