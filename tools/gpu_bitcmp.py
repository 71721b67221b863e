"""Developer utility: the same scenes stepped with two libraries (LIB_A, LIB_B = directories of library variants, tools/build_variant.sh; default:
tools/tmp_libs/base against the in-tree libraries), results compared bit for bit. A refactor that keeps every particle's arithmetic must print zeros.
The children take their library through WGS_LIB_DIR; the in-tree libraries are never touched."""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.join(ROOT, "wgsparkl_amd", "csrc")
if len(sys.argv) > 1 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import pipeline
    from wgsparkl_amd import MpmData, scenes
    name, out, steps = sys.argv[2], sys.argv[3], int(sys.argv[4])
    if name == "sand3": sc = scenes.reference_sand3()
    elif name == "landed":
        sc = scenes.neo_hookean_cube(n_side=64, with_floor=True); sc["particles"].pos[:, 1] -= 5.7; sc["particles"].vel[:, 1] = -3.0
    elif name == "c3s": sc = scenes.config_scene("c3", n_side=64)
    else: sc = scenes.neo_hookean_cube(n_side=48, with_floor=True)
    pipe = pipeline(3)
    data = MpmData.from_scene(pipe, sc)
    pipe.step(data, steps); data.sync()
    p = data.read_particles()
    np.savez(out, pos=p.pos, vel=p.vel, F=p.def_grad, C=p.affine, dp=p.dp_state, aff=p.cdf_affinity, nrm=p.cdf_normal, dist=p.cdf_dist)
    sys.exit(0)
dirs = [os.path.abspath(os.environ.get("LIB_A", os.path.join(ROOT, "tools", "tmp_libs", "base"))), os.path.abspath(os.environ.get("LIB_B", TREE))]
with tempfile.TemporaryDirectory() as tmp:
    for name, steps in (("sand3", 150), ("landed", 260), ("c3s", 60), ("cube", 40)):
        outs = []
        for tag, lib_dir in zip("ab", dirs):     # each child is a fresh process; check=True ends the run at the first one that fails
            out = os.path.join(tmp, f"{name}_{tag}.npz")
            subprocess.run(["timeout", "-k", "10", "300", sys.executable, __file__, "--child", name, out, str(steps)], check=True,
                           env={**os.environ, "WGS_LIB_DIR": lib_dir}, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            outs.append(np.load(out))
        a, b = outs
        print(name, steps, {k: int((a[k] != b[k]).sum()) for k in a.files}, "max |dpos|", float(np.abs(a["pos"] - b["pos"]).max()), flush=True)
