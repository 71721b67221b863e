#!/usr/bin/env python3
"""Developer utility (GPU): what removing particles at run time costs, one process, the variants of one scene alternating.

    timeout -k 10 600 python tools/gpu_remove_prof.py [c2] [fluid] [--json FILE]      (no part named: both)

c2      the C2 cube (1 M particles), fluid: a 2 M Tait fluid block without a floor. Per scene, created once each and timed in turn:
        plain           the scene as it is: what it launched before
        sink_nothing    the same with one box sink far away from every particle, period 1: every substep marks, waits for the stream
                        and reads the counts back; nothing is removed, nothing rebuilt
        sink_few        gpu_emit_prof.py's emitter (4 x 1 x 4 particles above the body every 8 substeps, falling at 1/16 cell per substep)
                        and a box sink of period 8 just below the nozzle, which takes the layer emitted 8 substeps earlier: one substep in
                        8 removes 16 particles, emits 16 and rebuilds the table; the particle count stays where it is
us per substep: wall clock over `k` substeps between two wgs_sync, median [min, max] of the repetitions; the difference to `plain` of
the same repetition is reported as well — for sink_few, 8 times that difference is the cost of a removing (and emitting) substep over an
ordinary one (`per_removing_substep_us`). Last, on a copy of `plain`: the wall time of ONE explicit remove_particles of a random 10 %
(`remove_10_percent_ms`, mask upload, compaction and the kept_from download included) and of the substep that follows it."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wgsparkl_amd import MpmData, MpmPipeline, scenes  # noqa: E402
from wgsparkl_amd.models import Emitter, Sink  # noqa: E402
from wgsparkl_amd.solver import ParticleSet  # noqa: E402

OUT = {}
WARM, K, REPS, PERIOD = 100, 200, 7, 8


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
    h = sc["cell_width"]
    if name == "plain":
        return MpmData.from_scene(pipe, sc)
    if name == "sink_nothing":
        far = tuple(float(x) + 1000.0 * h for x in ps.pos.max(0))
        return MpmData.from_scene(pipe, sc, sinks=[Sink.box(far, (h, h, h), period=1)])
    top = ps.pos.max(0)
    lo = tuple(float(x) for x in (ps.pos.mean(0)[0], top[1] + 2.0 * h, ps.pos.mean(0)[2]))
    proto = one_particle(ps)                       # (the scene's own material: the uniform layouts hold it)
    proto.vel[:] = 0.0
    proto.vel[0, 1] = -h / 16.0 / sc["params"].dt
    em = Emitter.nozzle(proto, lo, (4, 1, 4), h / 2.0, sc["params"].dt, jitter=0.1, seed=1)
    assert em.period == PERIOD
    # the layer emitted 8 substeps ago has fallen half a cell: it lies in [lo_y - h/2, lo_y], and the new one is not there yet
    sink = Sink.box((lo[0] + h, lo[1] - 0.25 * h, lo[2] + h), (1.5 * h, 0.3 * h, 1.5 * h), period=PERIOD)
    return MpmData.from_scene(pipe, sc, particle_capacity=ps.n + 64, emitters=[em], sinks=[sink])


def ab(pipe, tag, sc):
    datas = {name: make(pipe, sc, name) for name in ("plain", "sink_nothing", "sink_few")}
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
    few = datas["sink_few"]
    rec["sink_few"]["removed"] = int(sum(few.sink_counts()))
    rec["sink_few"]["emitted"], rec["sink_few"]["skipped_batches"] = [int(sum(x)) for x in few.emitter_counts()]
    rec["sink_few"]["per_removing_substep_us"] = {k: PERIOD * v for k, v in rec["sink_few"]["over_plain_us"].items()}
    # one explicit removal of a random 10 %, and the substep behind it (which rebuilds the table)
    d = datas["plain"]
    n = d.n
    mask = np.random.default_rng(1).uniform(size=n) < 0.1
    d.sync()
    t0 = time.perf_counter()
    kept_from = d.remove_particles(mask)
    t1 = time.perf_counter()
    pipe.step(d, 1)
    d.sync()
    t2 = time.perf_counter()
    rec["explicit"] = dict(n_before=int(n), removed=int(mask.sum()), n_after=int(d.n), kept_from_ok=bool(np.array_equal(kept_from, np.flatnonzero(~mask))),
                           remove_10_percent_ms=(t1 - t0) * 1e3, substep_after_us=(t2 - t1) * 1e6)
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
