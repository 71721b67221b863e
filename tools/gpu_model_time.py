"""developer utility: a bench configuration with another constitutive model (0 corotated, 1 neo-Hookean, 2 Tait fluid: lambda read as the bulk modulus, mu as the viscosity), event-free wall time per substep
and the event-timed fused G2P. With --table the models are PER PARTICLE (MpmData.set_particle_models): `all` labels every particle MODEL, `half:A` labels a random half MODEL
and the other half A, `thirds` deals 0 / 1 / 2 at random (MODEL is then the data's own model, which the table overrides).
usage: gpu_model_time.py c3 1 [substeps] [--n-side N] [--table all|half:A|thirds] [--json FILE]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from helpers import pipeline
from wgsparkl_amd import MpmData, scenes
ap = argparse.ArgumentParser()
ap.add_argument("cfg"); ap.add_argument("model", type=int); ap.add_argument("substeps", type=int, nargs="?", default=100)
ap.add_argument("--n-side", type=int, default=None); ap.add_argument("--table", default=None); ap.add_argument("--json", default=None)
a = ap.parse_args()
cfg, model, ksub = a.cfg, a.model, a.substeps
sc = scenes.config_scene(cfg, n_side=a.n_side)
pipe = pipeline(3)
n = sc["particles"].n
table = None
if a.table == "all":
    table = np.full(n, model, np.uint8)
elif a.table and a.table.startswith("half:"):
    table = np.where(np.random.default_rng(5).random(n) < 0.5, model, int(a.table[5:])).astype(np.uint8)
elif a.table == "thirds":
    table = np.random.default_rng(6).integers(0, 3, n).astype(np.uint8)
elif a.table:
    sys.exit(__doc__)
d = MpmData.from_scene(pipe, sc, model=model if table is None else (model + 1) % 2, models=table)
pipe.step(d, 40); d.sync()
tag = f"{cfg} model {model}" + (f" table {a.table}" if a.table else "")
reps = []
for rep in range(3):
    t0 = time.perf_counter(); pipe.step(d, ksub); d.sync()
    wall = (time.perf_counter() - t0) * 1e6 / ksub
    pipe.step(d, 40, True); d.sync()
    t = d.read_timings()
    g2p = (t["g2p"] + t["particles_update"]) * 1e3 / 40
    reps.append(dict(substep_us=round(wall, 1), g2p_us=round(g2p, 1)))
    print(f"{tag}: {wall:.1f} us/substep, fused G2P {g2p:.1f} us (event-timed, with its marks)", flush=True)
if a.json:
    with open(a.json, "a") as f:
        f.write(json.dumps(dict(case=tag, particles=n, reps=reps, overflow=d.stats()["overflow"])) + "\n")
