"""-m "not gpu": the Eulerian field output (include/wgsparkl_hip.h) as far as a box without a GPU sees it: the header says how a
binding detects it; calling the four entry points without a usable handle fails through the status path; the Python mirror has its
methods. The layout of wgs_grid_sample, the prototypes and the mirrors are tests/test_abi.py. No compute call is made here."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_tells_a_binding_how_to_detect_the_feature():
    header = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()
    assert "detect wgs_sample_grid by symbol lookup" in header


@pytest.mark.parametrize("dim", [2, 3])
def test_calls_without_a_handle_fail_through_the_status_path(hip_libs, dim):
    """No wgs_data can be created without a GPU (wgs_pipeline_create fails with WGS_ERR_NO_DEVICE there), so what a CPU-only box can
    show is the argument check in front of everything else: a NULL handle is WGS_ERR_INVALID_ARGUMENT with a message, not a crash, and
    nothing is written."""
    lib, T = hip_libs.load(dim)
    pts = (C.c_float * (4 * dim))()
    out = (T.GridSample * 4)()
    lo = (C.c_int32 * dim)()
    dims = (C.c_uint32 * dim)(*([2] * dim))
    win = (C.c_float * (2 ** dim * (dim + 1)))(*([7.0] * (2 ** dim * (dim + 1))))
    calls = [lambda: lib.wgs_sample_grid(None, pts, 4, out), lambda: lib.wgs_sample_grid_device(None, None, 4, None),
             lambda: lib.wgs_read_grid_window(None, lo, dims, win), lambda: lib.wgs_read_grid_window_device(None, lo, dims, None)]
    for call in calls:
        assert call() == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(out) == bytes(C.sizeof(out)) and all(x == 7.0 for x in win)


def test_python_mirror_has_the_four_methods():
    from wgsparkl_amd.pipeline import GridSamples, MpmData
    for m in ("sample_grid", "grid_window", "sample_grid_device", "grid_window_device"):
        assert callable(getattr(MpmData, m))
    assert [f for f in GridSamples.__dataclass_fields__][:4] == ["velocity", "velocity_gradient", "density", "active_nodes"]
