"""-m gpu: a run whose libraries come from WGS_LIB_DIR computes what the in-tree libraries compute. The 512-particle
neo-Hookean cube, two substeps, in two fresh child processes (the override is read once per process), each under its own
time limit: one with WGS_LIB_DIR pointing at a copy of the tree's libraries, one with it unset. The positions are equal
bit for bit, and the override child says on stderr where its library came from."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = ("import hashlib\n"
         "from wgsparkl_amd import MpmData, MpmPipeline, scenes\n"
         "sc = scenes.neo_hookean_cube(n_side=8)\n"
         "pipe = MpmPipeline(0, 3)\n"
         "data = MpmData.new(pipe, sc['params'], sc['particles'], sc['colliders'], sc['cell_width'], sc['grid_capacity'], sc['model'])\n"
         "pipe.step(data, 2)\n"
         "data.sync()\n"
         "pos = data.read_positions()\n"
         "print('positions', pos.shape[0], hashlib.sha256(pos.tobytes()).hexdigest())\n")


def child(lib_dir):
    env = {k: v for k, v in os.environ.items() if k != "WGS_LIB_DIR"}
    if lib_dir is not None:
        env["WGS_LIB_DIR"] = lib_dir
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [ln for ln in r.stdout.split("\n") if ln.startswith("positions ")][-1], r.stderr


@pytest.mark.gpu
def test_a_copy_of_the_libraries_chosen_by_path_computes_the_same_positions(hip_libs, tmp_path):
    for dim in (2, 3):
        shutil.copy(hip_libs.lib_path(dim), tmp_path / os.path.basename(hip_libs.lib_path(dim)))
    with_override, said = child(str(tmp_path))
    assert "WGS_LIB_DIR" in said and str(tmp_path) in said, said
    without, said = child(None)
    assert "WGS_LIB_DIR" not in said
    assert with_override.split()[1] == "512"
    assert with_override == without
