"""include/wgsparkl_hip.hpp — the C++ host-side mirror of the reference's Rust API over the C ABI (the reference's host
is compiled code; there is no Rust toolchain in this image). Built with g++ against the in-tree library."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, hip_libs):
    libdir = os.path.dirname(hip_libs.lib_path(3))
    exe = tmp_path / "host_mirror"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/include", f"{ROOT}/tests/cpp/host_mirror.cpp",
                    f"-L{libdir}", "-lwgsparkl3d_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)], check=True)
    return exe


def test_cpp_mirror_compiles_and_refuses_to_run_without_a_gpu(hip_libs, tmp_path):
    """The header compiles warning-free as C++17 and links against the C ABI. On a box without a GPU
    MpmPipeline::create throws WGS_ERR_NO_DEVICE: there is no CPU fallback behind the C++ surface either."""
    import torch
    exe = _build(tmp_path, hip_libs)
    r = subprocess.run([str(exe), "nodevice"], capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 3, r.stdout          # a pipeline could be created
    else:
        assert r.returncode == 0 and f"status {hip_libs.ERR_NO_DEVICE}" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mirror_runs_the_reference_smoke_scene(hip_libs, tmp_path):
    """The scene of the reference's own smoke test (src/pipeline.rs:302-331) written against the C++ mirror exactly as
    the Rust test writes it, 10 substeps: bit-identical positions to the Python mirror on the same library."""
    from helpers import run_gpu
    from wgsparkl_amd import scenes
    exe = _build(tmp_path, hip_libs)
    out = tmp_path / "pos.bin"
    r = subprocess.run([str(exe), "smoke", str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=np.float32).reshape(-1, 3)
    ref = run_gpu(scenes.reference_smoke_scene(), 10).read_particles().pos
    assert got.shape == ref.shape == (1000, 3)
    assert np.array_equal(got, ref)
