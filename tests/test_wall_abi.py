"""-m "not gpu": the C ABI of the domain walls (include/wgsparkl_hip.h): wgs_wall has the size and the field offsets the header
compiles to, in both dimensions; the two entry points are exported with full prototypes, next to wgs_set_grid_growth; every mirror
declares them; calling them without a usable handle fails through the status path. No compute call is made here."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wgs_set_domain_walls", "wgs_get_domain_walls")
FIELDS = ("type", "friction", "plane")


@pytest.mark.parametrize("dim", [2, 3])
def test_wall_layout_matches_the_header(hip_libs, dim, tmp_path):
    assert C.sizeof(hip_libs.Wall) == 12
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#define WGS_DIM {dim}', '#include "wgsparkl_hip.h"', 'int main(void) {',
             '  printf("%zu", sizeof(wgs_wall));']
    lines += [f'  printf(" %zu", offsetof(wgs_wall, {f}));' for f in FIELDS]
    lines += ['  printf(" %d %d %d %d", WGS_WALL_NONE, WGS_WALL_STICKY, WGS_WALL_SLIP, WGS_WALL_SEPARATE);', '  printf("\\n");', '  return 0; }']
    src, exe = tmp_path / "wall_abi.c", tmp_path / "wall_abi"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(ROOT, 'include')}", str(src), "-o", str(exe)], check=True)
    seen = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert seen[0] == C.sizeof(hip_libs.Wall) == 12
    assert seen[1:4] == [getattr(hip_libs.Wall, f).offset for f in FIELDS] == [0, 4, 8]
    assert seen[4:] == [hip_libs.WALL_NONE, hip_libs.WALL_STICKY, hip_libs.WALL_SLIP, hip_libs.WALL_SEPARATE] == [0, 1, 2, 3]
    from wgsparkl_amd import models
    assert [models.WALL_NONE, models.WALL_STICKY, models.WALL_SLIP, models.WALL_SEPARATE] == seen[4:]


@pytest.mark.parametrize("dim", [2, 3])
def test_the_two_symbols_are_exported_with_prototypes(hip_libs, dim):
    lib, T = hip_libs.load(dim)
    names = list(hip_libs.prototypes(T))
    at = names.index("wgs_set_grid_growth")
    assert names[at + 1:at + 3] == list(NAMES), "the two prototypes stand behind wgs_set_grid_growth, in the header's order"
    for name in NAMES:
        fn = getattr(lib, name)                     # (AttributeError: the library does not export it)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == 2
    assert lib.wgs_abi_version() == 7


def test_the_header_tells_a_binding_how_to_detect_the_feature():
    header = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()
    assert "#define WGS_ABI_VERSION 7" in header
    assert "detect wgs_set_domain_walls by symbol lookup" in header
    assert header.index("wgs_set_grid_growth(") < header.index("wgs_set_domain_walls(") < header.index("wgs_get_domain_walls(") < header.index("wgs_debug_scan(")
    assert "axis 0 low, axis 0 high, axis 1 low" in header, "the header states the order in which a corner node takes the faces"
    for said in ("AFTER the walls", "WGS_PASS_GRID_UPDATE", "(low.plane - 1.5) h"):
        assert said in header, said
    hpp = open(os.path.join(ROOT, "include", "wgsparkl_hip.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "wgsparkl-hip-sys", "src", "lib.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name + "(" in hpp and "pub fn " + name + "(" in rs and name in integration, name
    assert "pub struct wgs_wall" in rs
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
        assert call() == 1                                   # WGS_ERR_INVALID_ARGUMENT
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
