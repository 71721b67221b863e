"""-m "not gpu": the Lagrangian field output (include/wgsparkl_hip.h) as far as a box without a GPU sees it: where the header puts the
section; calling the two entry points without a usable handle fails through the status path; the Python mirror has its methods. The
layout of wgs_particle_field, the prototypes and the mirrors are tests/test_abi.py. No compute call is made here."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("stress", "mean_stress", "von_mises", "volume_ratio", "stretch", "model")


def test_the_header_tells_a_binding_how_to_detect_the_feature():
    header = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()
    assert "detect wgs_read_particle_fields by symbol lookup" in header
    assert header.index("Lagrangian field output") < header.index("Eulerian field output"), "the new section stands in front of the Eulerian one"
    assert header.index("wgs_enqueue_diagnostics(") < header.index("wgs_read_particle_fields(") < header.index("wgs_sample_grid(")


@pytest.mark.parametrize("dim", [2, 3])
def test_calls_without_a_handle_fail_through_the_status_path(hip_libs, dim):
    """No wgs_data can be created without a GPU, so what a CPU-only box can show is the argument check in front of everything else: a
    NULL handle is WGS_ERR_INVALID_ARGUMENT with a message, not a crash, and nothing is written."""
    lib, T = hip_libs.load(dim)
    out = (T.ParticleField * 4)()
    C.memset(out, 0x5a, C.sizeof(out))
    for call in (lambda: lib.wgs_read_particle_fields(None, out), lambda: lib.wgs_read_particle_fields_device(None, None),
                 lambda: lib.wgs_read_particle_fields(None, None)):
        assert call() == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(out) == b"\x5a" * C.sizeof(out)


def test_python_mirror_has_the_two_methods():
    from wgsparkl_amd.pipeline import MpmData, ParticleFields
    for m in ("particle_fields", "particle_fields_device"):
        assert callable(getattr(MpmData, m))
    assert [f for f in ParticleFields.__dataclass_fields__][:6] == list(FIELDS)
