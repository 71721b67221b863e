"""-m "not gpu": the C ABI of the Eulerian field output (include/wgsparkl_hip.h): wgs_grid_sample has the size and the field
offsets the header compiles to, in both dimensions; the four entry points are exported with full prototypes; every mirror
declares them; calling them without a usable handle fails through the status path. No compute call is made here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wgs_sample_grid", "wgs_sample_grid_device", "wgs_read_grid_window", "wgs_read_grid_window_device")
FIELDS = ("velocity", "velocity_gradient", "density", "active_nodes")


@pytest.mark.parametrize("dim,words", [(3, 14), (2, 8)])
def test_grid_sample_layout_matches_the_header(hip_libs, dim, words, tmp_path):
    _, T = hip_libs.load(dim)
    assert C.sizeof(T.GridSample) == 4 * words == 4 * (dim + dim * dim + 2)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#define WGS_DIM {dim}', '#include "wgsparkl_hip.h"', 'int main(void) {',
             '  printf("%zu", sizeof(wgs_grid_sample));']
    lines += [f'  printf(" %zu", offsetof(wgs_grid_sample, {f}));' for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0; }']
    src, exe = tmp_path / "probe_abi.c", tmp_path / "probe_abi"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    seen = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert seen[0] == C.sizeof(T.GridSample)
    assert seen[1:] == [getattr(T.GridSample, f).offset for f in FIELDS]


@pytest.mark.parametrize("dim", [2, 3])
def test_the_four_symbols_are_exported_with_prototypes(hip_libs, dim):
    lib, T = hip_libs.load(dim)
    protos = hip_libs.prototypes(T)
    assert list(protos)[-4:] == list(NAMES), "the four prototypes close the table, in the header's order"
    for name in NAMES:
        fn = getattr(lib, name)                     # (AttributeError: the library does not export it)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == 4
    assert lib.wgs_abi_version() == 7


def test_the_header_tells_a_binding_how_to_detect_the_feature():
    header = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()
    assert "#define WGS_ABI_VERSION 7" in header
    assert "detect wgs_sample_grid by symbol lookup" in header
    hpp = open(os.path.join(ROOT, "include", "wgsparkl_hip.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "wgsparkl-hip-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert name + "(" in hpp and "pub fn " + name + "(" in rs, name
    assert "pub struct wgs_grid_sample" in rs


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
        assert call() == 1                                   # WGS_ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(out) == bytes(C.sizeof(out)) and all(x == 7.0 for x in win)


def test_python_mirror_has_the_four_methods():
    from wgsparkl_amd.pipeline import GridSamples, MpmData
    for m in ("sample_grid", "grid_window", "sample_grid_device", "grid_window_device"):
        assert callable(getattr(MpmData, m))
    assert [f for f in GridSamples.__dataclass_fields__][:4] == ["velocity", "velocity_gradient", "density", "active_nodes"]
