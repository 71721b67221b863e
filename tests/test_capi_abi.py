"""-m "not gpu": the header declares the surface the reference's call sites need and cites them; creating a pipeline without a GPU
fails loudly (no CPU fallback); the product never references the oracle. That the libraries export what the header declares and
that every mirror has its layouts is tests/test_abi.py. No compute call is made here."""
import ctypes as C
import os
import re

import pytest

import abi

ROOT = abi.ROOT


def test_header_declares_the_expected_surface():
    must = {"wgs_pipeline_create", "wgs_data_create", "wgs_step", "wgs_sync", "wgs_set_sim_params",
            "wgs_set_collider_poses", "wgs_set_body_velocities", "wgs_read_positions", "wgs_read_particles",
            "wgs_read_grid", "wgs_read_blocks", "wgs_read_timings", "wgs_get_stats", "wgs_data_destroy",
            "wgs_pipeline_destroy", "wgs_last_error", "wgs_dim", "wgs_set_constitutive_model"}
    assert must <= set(abi.header().functions)
    # every entry point cites the reference interface it replaces
    text = abi.read(abi.HEADER_PATH)
    assert text.count("src/pipeline.rs") >= 5 and "src_testbed/step.rs" in text


def test_no_cpu_fallback(hip_libs):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib, _ = hip_libs.load(3)
    h = C.c_void_p()
    st = lib.wgs_pipeline_create(0, C.byref(h))
    assert st == hip_libs.ERR_NO_DEVICE and not h.value
    assert b"no HIP device" in lib.wgs_last_error()
    from wgsparkl_amd import MpmPipeline
    from wgsparkl_amd._ffi import WgsError
    with pytest.raises(WgsError):
        MpmPipeline(0, 3)


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under wgsparkl_amd/ or include/ may reference it."""
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "wgsparkl_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".sh")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                if re.search(r"(from|import)\s+oracle\b|oracle/|mpm_oracle|liborc", txt):
                    bad.append(os.path.join(base, f))
    assert not bad, bad
