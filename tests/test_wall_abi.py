"""-m "not gpu": the domain walls (include/wgsparkl_hip.h) as far as a box without a GPU sees them: what the header says about
them and where the documents name them; calling the two entry points without a usable handle fails through the status path; the
Python mirror and the scenes. The layout of wgs_wall, the WGS_WALL_* values, the prototypes and the mirrors are tests/test_abi.py.
No compute call is made here."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wgs_set_domain_walls", "wgs_get_domain_walls")


def test_the_header_tells_a_binding_how_to_detect_the_feature():
    header = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()
    assert "detect wgs_set_domain_walls by symbol lookup" in header
    assert header.index("wgs_set_grid_growth(") < header.index("wgs_set_domain_walls(") < header.index("wgs_get_domain_walls(") < header.index("wgs_debug_scan(")
    assert "axis 0 low, axis 0 high, axis 1 low" in header, "the header states the order in which a corner node takes the faces"
    for said in ("AFTER the walls", "WGS_PASS_GRID_UPDATE", "(low.plane - 1.5) h"):
        assert said in header, said
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in integration, name
    for doc in ("README.md", "DESIGN.md"):
        assert "wgs_set_domain_walls" in open(os.path.join(ROOT, doc)).read(), doc


@pytest.mark.parametrize("dim", [2, 3])
def test_calls_without_a_handle_fail_through_the_status_path(hip_libs, dim):
    """No wgs_data can be created without a GPU, so what a CPU-only box can show is the argument check in front of everything else: a
    NULL handle is WGS_ERR_INVALID_ARGUMENT with a message, not a crash, and nothing is written."""
    lib, _ = hip_libs.load(dim)
    walls = (hip_libs.Wall * (2 * dim))()
    C.memset(walls, 0x5a, C.sizeof(walls))
    for call in (lambda: lib.wgs_set_domain_walls(None, walls), lambda: lib.wgs_set_domain_walls(None, None),
                 lambda: lib.wgs_get_domain_walls(None, walls), lambda: lib.wgs_get_domain_walls(None, None)):
        assert call() == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(walls) == b"\x5a" * C.sizeof(walls)


def test_python_mirror_has_the_methods_and_the_wall_helpers():
    from wgsparkl_amd import Wall, scenes
    from wgsparkl_amd.models import WALL_SLIP, WALL_STICKY
    from wgsparkl_amd.pipeline import MpmData
    for m in ("set_domain_walls", "domain_walls"):
        assert callable(getattr(MpmData, m))
    assert Wall.low(2.0, 1.0).plane == 2 and Wall.low(2.5, 1.0).plane == 2 and Wall.low(-0.6, 0.3).plane == -2
    assert Wall.high(2.0, 1.0).plane == 2 and Wall.high(2.5, 1.0).plane == 3 and Wall.high(-0.7, 0.3).plane == -2
    assert Wall.low(1.0, 1.0, WALL_STICKY, 0.25) == Wall(WALL_STICKY, 0.25, 1) and Wall().type == WALL_SLIP


def test_the_default_tank_scenes_are_what_they_were_and_the_grid_form_has_no_colliders():
    from wgsparkl_amd import scenes
    for make, ncol, faces in ((scenes.dam_break, 2, 6), (lambda **kw: scenes.block_in_fluid(dim=3, **kw), 5, 6),
                              (lambda **kw: scenes.block_in_fluid(dim=2, **kw), 3, 4)):
        a, b, g = make(), make(walls="colliders"), make(walls="grid")
        assert "walls" not in a and len(a["colliders"]) == ncol and sorted(a) == sorted(b)
        assert g["colliders"] == [] and len(g["walls"]) == faces and sum(w is not None for w in g["walls"]) == ncol
        assert a["particles"].pos.tobytes() == g["particles"].pos.tobytes()
    with pytest.raises(ValueError):
        scenes.dam_break(walls="none")
    for dim in (2, 3):
        sc = scenes.walled_box(dim, n=500)
        assert sc["colliders"] == [] and len(sc["walls"]) == 2 * dim and sc["particles"].dim == dim
        assert scenes.walled_box(dim, n=500, with_walls=False)["walls"] is None
