"""-m "not gpu": the C ABI of the Lagrangian field output (include/wgsparkl_hip.h): wgs_particle_field has the size and the field
offsets the header compiles to, in both dimensions; the two entry points are exported with full prototypes, in front of the Eulerian
four; every mirror declares them; calling them without a usable handle fails through the status path. No compute call is made here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wgs_read_particle_fields", "wgs_read_particle_fields_device")
FIELDS = ("stress", "mean_stress", "von_mises", "volume_ratio", "stretch", "model")


@pytest.mark.parametrize("dim,size", [(3, 64), (2, 40)])
def test_particle_field_layout_matches_the_header(hip_libs, dim, size, tmp_path):
    _, T = hip_libs.load(dim)
    assert C.sizeof(T.ParticleField) == size == 4 * (dim * dim + dim + 4)
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#define WGS_DIM {dim}', '#include "wgsparkl_hip.h"', 'int main(void) {',
             '  printf("%zu", sizeof(wgs_particle_field));']
    lines += [f'  printf(" %zu", offsetof(wgs_particle_field, {f}));' for f in FIELDS]
    lines += ['  printf("\\n");', '  return 0; }']
    src, exe = tmp_path / "field_abi.c", tmp_path / "field_abi"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    seen = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert seen[0] == C.sizeof(T.ParticleField)
    assert seen[1:] == [getattr(T.ParticleField, f).offset for f in FIELDS]


@pytest.mark.parametrize("dim", [2, 3])
def test_the_two_symbols_are_exported_with_prototypes(hip_libs, dim):
    lib, T = hip_libs.load(dim)
    protos = hip_libs.prototypes(T)
    assert list(protos)[-6:-4] == list(NAMES), "the two prototypes stand in front of the Eulerian four, in the header's order"
    for name in NAMES:
        fn = getattr(lib, name)                     # (AttributeError: the library does not export it)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == 2
    assert lib.wgs_abi_version() == 7


def test_the_header_tells_a_binding_how_to_detect_the_feature():
    header = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()
    assert "#define WGS_ABI_VERSION 7" in header
    assert "detect wgs_read_particle_fields by symbol lookup" in header
    assert header.index("Lagrangian field output") < header.index("Eulerian field output"), "the new section stands in front of the Eulerian one"
    assert header.index("wgs_enqueue_diagnostics(") < header.index("wgs_read_particle_fields(") < header.index("wgs_sample_grid(")
    hpp = open(os.path.join(ROOT, "include", "wgsparkl_hip.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "wgsparkl-hip-sys", "src", "lib.rs")).read()
    for name in NAMES:
        assert name + "(" in hpp and "pub fn " + name + "(" in rs, name
    assert "pub struct wgs_particle_field" in rs


@pytest.mark.parametrize("dim", [2, 3])
def test_calls_without_a_handle_fail_through_the_status_path(hip_libs, dim):
    """No wgs_data can be created without a GPU, so what a CPU-only box can show is the argument check in front of everything else: a
    NULL handle is WGS_ERR_INVALID_ARGUMENT with a message, not a crash, and nothing is written."""
    lib, T = hip_libs.load(dim)
    out = (T.ParticleField * 4)()
    C.memset(out, 0x5a, C.sizeof(out))
    for call in (lambda: lib.wgs_read_particle_fields(None, out), lambda: lib.wgs_read_particle_fields_device(None, None),
                 lambda: lib.wgs_read_particle_fields(None, None)):
        assert call() == 1                                   # WGS_ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(out) == b"\x5a" * C.sizeof(out)


def test_python_mirror_has_the_two_methods():
    from wgsparkl_amd.pipeline import MpmData, ParticleFields
    for m in ("particle_fields", "particle_fields_device"):
        assert callable(getattr(MpmData, m))
    assert [f for f in ParticleFields.__dataclass_fields__][:6] == list(FIELDS)
