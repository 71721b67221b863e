"""-m "not gpu": the force-field extension (include/wgsparkl_hip_forces.h) as far as a box without a GPU sees it. tests/test_abi.py
holds the MAIN header to its table and every mirror to exactly that table, so the extension is held here: the struct's layout from a
compiled C probe through the main header alone, both dimensions; the declarations and the rule's sentences, verbatim; the ctypes
twin and prototypes; the Rust file's struct, constants and functions against the extension header with tests/abi.py's parser; both
functions wrapped by the C++ header; NULL-argument statuses; the Python mirror; the default scenes unchanged. No compute call is made."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi

EXT_PATH = os.path.join(abi.INCLUDE, "wgsparkl_hip_forces.h")
RUST_PATH = os.path.join(abi.ROOT, "rust", "wgsparkl-hip-sys", "src", "forces.rs")
EXT = abi.header(abi.read(EXT_PATH))
FIELDS = ["kind", "falloff", "region", "strength", "softening", "center", "vec", "region_center", "region_half"]
CONSTANTS = dict(WGS_FORCE_NONE=0, WGS_FORCE_UNIFORM=1, WGS_FORCE_RADIAL=2, WGS_FORCE_VORTEX=3, WGS_FORCE_DRAG=4,
                 WGS_REGION_ALL=0, WGS_REGION_BOX=1, WGS_REGION_BALL=2, WGS_MAX_FORCE_FIELDS=8)
OFFSETS = dict(kind=(0, 4), falloff=(4, 4), region=(8, 4), strength=(12, 4), softening=(16, 4), center=(20, 12), vec=(32, 12),
               region_center=(44, 12), region_half=(56, 12))
DECLARATIONS = (
    "enum { WGS_FORCE_NONE = 0, WGS_FORCE_UNIFORM = 1, WGS_FORCE_RADIAL = 2, WGS_FORCE_VORTEX = 3, WGS_FORCE_DRAG = 4 };",
    "enum { WGS_REGION_ALL = 0, WGS_REGION_BOX = 1, WGS_REGION_BALL = 2 };",
    "#define WGS_MAX_FORCE_FIELDS 8",
    "wgs_status wgs_set_force_fields(wgs_data *data, const wgs_force_field *fields /* n, or NULL with n == 0 */, uint32_t n);",
    "wgs_status wgs_get_force_fields(wgs_data *data, wgs_force_field *out /* WGS_MAX_FORCE_FIELDS */, uint32_t *n);",
)
RULE = (
    "w_p(q), p = falloff in {0,1,2,3}:   1,  1/sqrt(q),  1/q,  1/(q sqrt(q))",
    "UNIFORM  v += dt * vec",
    "RADIAL   r = center - x;  q = |r|^2 + softening^2;   v += dt * strength * w_p(q) * r      (strength > 0 attracts)",
    "VORTEX   r = x - center;  rp = r - (r.n) n;  q = |rp|^2 + softening^2;",
    "v += dt * strength * w_p(q) * (n x rp)",
    "3D: n = vec normalised once on the host in double",
    "2D: n = +z, i.e. (-r_y, r_x)",
    "DRAG     kdt = min(strength * dt, 1e30);  s = kdt / (1 + kdt);  v += s * (vec - v)",
    "x_k = (float)cell_k * h, with cell_k = block_k * BW + local_k",
    "dt = the device's SimParamsDev::dt, as the grid update reads it. wgs_set_sim_params carries over.",
    "|x_k - region_center_k| <= region_half_k on every axis",
    "|x - region_center|^2 <= region_half[0]^2. This is a disc in 2D.",
)


def test_the_extension_header_declares_exactly_the_feature():
    assert EXT.structs == {"wgs_force_field": FIELDS}
    assert EXT.constants == list(CONSTANTS) and list(EXT.functions) == ["wgs_set_force_fields", "wgs_get_force_fields"]
    text = abi.read(EXT_PATH)
    for line in DECLARATIONS + RULE:
        assert line in text, line
    for said in ("no device memory", "NOT part of a checkpoint", "WGS_PASS_GRID_UPDATE", "IN FRONT OF the domain walls", "mass > 0",
                 "not written", "kept and skipped", "removes every field", "refusals change nothing"):
        assert said in text, said
    main = abi.read(abi.HEADER_PATH)
    flat = " ".join(main.replace("\n *", " ").split())
    assert "and, still 7, the force-field extension of wgsparkl_hip_forces.h — detect wgs_set_force_fields by symbol lookup" in flat
    assert main.index("wgs_get_plasticity_model(") < main.index('#include "wgsparkl_hip_forces.h"') < main.index("wgs_debug_scan(")
    # the main header's own table does not grow: the extension's names are not in it
    hdr = abi.header()
    assert "wgs_force_field" not in hdr.structs and not set(CONSTANTS) & set(hdr.constants) and not set(EXT.functions) & set(hdr.functions)
    build = abi.read(os.path.join(abi.ROOT, "wgsparkl_amd", "csrc", "build.sh"))
    assert "../../include/wgsparkl_hip_forces.h" in build.split("sources=")[1].splitlines()[0], "a changed extension header must rebuild the libraries"


@pytest.mark.parametrize("dim", [2, 3])
def test_struct_layout_from_a_compiled_probe_through_the_main_header_alone(dim, tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "wgsparkl_hip.h"', "int main(void) {",
             '  printf("S %zu\\n", sizeof(wgs_force_field));']
    lines += [f'  printf("F {f} %zu %zu\\n", offsetof(wgs_force_field, {f}), sizeof(((wgs_force_field *)0)->{f}));' for f in FIELDS]
    lines += [f'  printf("C {c} %lld\\n", (long long)({c}));' for c in CONSTANTS]
    lines += ["  wgs_status (*set)(wgs_data *, const wgs_force_field *, uint32_t) = wgs_set_force_fields;",
              "  wgs_status (*get)(wgs_data *, wgs_force_field *, uint32_t *) = wgs_get_force_fields;",
              "  return set == NULL || get == NULL;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    # (compiled, not linked against the library: the addresses are taken in a translation unit of their own)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-DWGS_DIM={dim}", f"-I{abi.INCLUDE}", "-c", str(src), "-o", str(tmp_path / "probe.o")], check=True)
    body = "\n".join(l for l in lines if "(*set)" not in l and "(*get)" not in l).replace("return set == NULL || get == NULL;", "return 0;")
    src.write_text(body + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-DWGS_DIM={dim}", f"-I{abi.INCLUDE}", str(src), "-o", str(exe)], check=True)
    out = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert ["S", "68"] in out
    assert {l[1]: (int(l[2]), int(l[3])) for l in out if l[0] == "F"} == OFFSETS
    assert {l[1]: int(l[2]) for l in out if l[0] == "C"} == CONSTANTS


def test_ctypes_twin_and_prototypes():
    from wgsparkl_amd import _ffi, models
    ct = _ffi.ForceField
    assert C.sizeof(ct) == 68 and [f for f, _ in ct._fields_] == FIELDS
    assert {f: (getattr(ct, f).offset, getattr(ct, f).size) for f in FIELDS} == OFFSETS
    protos = _ffi.forces_prototypes()
    assert list(protos) == list(EXT.functions)
    for name, (ret, params) in EXT.functions.items():
        restype, argtypes = protos[name]
        assert (abi.ctypes_kind(restype), [abi.ctypes_kind(t) for t in argtypes]) == (abi.return_kind(ret), abi.param_kinds(params)), name
    # ... and they stay out of the main header's table
    assert not set(protos) & set(_ffi.prototypes(_ffi.make_types(3))) and not set(protos) & set(_ffi.EXPORTS)
    for mod in (_ffi, models):
        for name, value in CONSTANTS.items():
            assert getattr(mod, name[4:]) == value, (mod.__name__, name)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_loaded_library_carries_the_prototypes(hip_libs, dim):
    lib, _ = hip_libs.load(dim)
    for name, (restype, argtypes) in hip_libs.forces_prototypes().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


@pytest.mark.parametrize("dim", [2, 3])
def test_rust_file_is_the_extension_headers(dim):
    text = abi.read(RUST_PATH)
    rust = abi.rust_layout(text, dim)
    assert rust.size == {"wgs_force_field": 68} and rust.fields["wgs_force_field"] == OFFSETS
    assert rust.const == CONSTANTS
    fns = abi.rust_functions(text)
    assert list(fns) == list(EXT.functions)
    for name, (ret, params) in EXT.functions.items():
        assert fns[name] == (abi.return_kind(ret), abi.param_kinds(params)), name
    lib_rs = abi.read(abi.RUST_PATH)
    assert "pub mod forces;" in lib_rs and "wgs_force_field" not in lib_rs.replace("pub mod forces;", "")


def test_cpp_wrapper_wraps_both():
    hpp = abi.read(abi.HPP_PATH)
    for name in EXT.functions:
        assert name + "(" in hpp, name
    assert "void set_force_fields(const std::vector<wgs_force_field> &fields)" in hpp and "std::vector<wgs_force_field> force_fields()" in hpp


@pytest.mark.parametrize("dim", [2, 3])
def test_calls_without_a_handle_fail_through_the_status_path(hip_libs, dim):
    """No wgs_data can be created without a GPU: a NULL handle is WGS_ERR_INVALID_ARGUMENT with a message, and nothing is written."""
    lib, _ = hip_libs.load(dim)
    arr = (hip_libs.ForceField * hip_libs.MAX_FORCE_FIELDS)()
    C.memset(arr, 0x5a, C.sizeof(arr))
    n = C.c_uint32(0x5a5a5a5a)
    for call in (lambda: lib.wgs_set_force_fields(None, arr, 1), lambda: lib.wgs_set_force_fields(None, None, 0),
                 lambda: lib.wgs_get_force_fields(None, arr, C.byref(n)), lambda: lib.wgs_get_force_fields(None, None, None)):
        assert call() == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(arr) == b"\x5a" * C.sizeof(arr) and n.value == 0x5a5a5a5a


def test_python_mirror():
    from wgsparkl_amd import models, scenes
    from wgsparkl_amd.models import ForceField
    from wgsparkl_amd.pipeline import MpmData
    for m in ("set_force_fields", "force_fields"):
        assert callable(getattr(MpmData, m))
    f = ForceField.radial((1.0, 2.0), 3.0, falloff=2, softening=0.5)
    assert (f.kind, f.falloff, f.region, f.strength, f.softening, f.center) == (models.FORCE_RADIAL, 2, models.REGION_ALL, 3.0, 0.5, (1.0, 2.0, 0.0))
    b = f.within_box((0.0, 1.0, 2.0), (3.0, 4.0, 5.0))
    assert (b.region, b.region_center, b.region_half, b.strength) == (models.REGION_BOX, (0.0, 1.0, 2.0), (3.0, 4.0, 5.0), 3.0) and f.region == models.REGION_ALL
    c = ForceField.drag(9.0, (1.0, 0.0, 0.0)).within_ball((1.0, 1.0, 1.0), 2.5)
    assert (c.kind, c.strength, c.vec, c.region, c.region_half[0]) == (models.FORCE_DRAG, 9.0, (1.0, 0.0, 0.0), models.REGION_BALL, 2.5)
    assert ForceField.uniform((0.0, -9.81)).vec == (0.0, -9.81, 0.0) and ForceField.vortex((0.0, 0.0), 2.0).vec == (0.0, 0.0, 1.0)
    assert ForceField().kind == models.FORCE_NONE
    assert "| `forces` |" in scenes.__doc__ and scenes.__doc__.index("| `walls` |") < scenes.__doc__.index("| `forces` |")
    for doc, said in (("INTEGRATION.md", "wgs_set_force_fields"), ("INTEGRATION.md", "wgs_get_force_fields"), ("README.md", "wgs_set_force_fields"),
                      ("DESIGN.md", "## 7e. Force fields"), ("DESIGN.md", "k_grid_forces"), ("tools/README.md", "gpu_forces_prof.py")):
        assert said in abi.read(os.path.join(abi.ROOT, doc)), (doc, said)


def test_the_new_scenes_and_the_default_scenes_unchanged():
    from wgsparkl_amd import scenes
    from wgsparkl_amd.models import FORCE_DRAG, FORCE_RADIAL, FORCE_VORTEX, REGION_BOX
    for dim in (2, 3):
        sc = scenes.planetoid(dim, radius=3.0)
        assert [f.kind for f in sc["forces"]] == [FORCE_RADIAL] and sc["colliders"] == [] and not any(sc["params"].gravity) and "walls" not in sc
        rel = sc["particles"].pos.astype(np.float64) - sc["centre"]
        assert np.linalg.norm(rel, axis=1).max() <= sc["start_radius"] and np.all((rel * sc["particles"].vel).sum(1) >= 0)
        assert np.allclose(sc["forces"][0].center[:dim], sc["centre"])
        ctl = scenes.planetoid(dim, radius=3.0, with_field=False)
        assert ctl["forces"] is None and ctl["particles"].pos.tobytes() == sc["particles"].pos.tobytes()
        sc = scenes.vortex_tank(dim, tank=(8, 6, 8))
        assert [f.kind for f in sc["forces"]] == [FORCE_VORTEX, FORCE_DRAG] and sc["forces"][1].region == REGION_BOX
        assert sum(w is not None for w in sc["walls"]) == 2 * dim - 1 and sc["colliders"] == [] and sc["particles"].dim == dim
    # no scene that existed gained the key
    for make in (scenes.dam_break, scenes.block_in_fluid, scenes.walled_box, scenes.snowball, scenes.reference_smoke_scene,
                 lambda: scenes.neo_hookean_cube(n_side=4), lambda: scenes.sand_column(4, 4, 4)):
        assert "forces" not in make()
