"""-m "not gpu": what include/wgsparkl_hip.h promises, asserted for EVERY struct, constant and function it declares (tests/abi.py reads
the list from the header, gcc answers for it) against the three hand-written mirrors: wgsparkl_amd/_ffi.py (ctypes),
rust/wgsparkl-hip-sys/src/lib.rs (never compiled: its repr(C) layout is computed) and include/wgsparkl_hip.hpp. A struct, constant or
entry point the next feature adds is covered without an edit here — or fails here until its mirrors exist. Each comparison is a
function that returns what it found wrong, so that the last tests can show it the mistakes it exists for, on copies in memory.
No compute call is made here."""
import ctypes as C
import os
import re

import pytest

import abi
from wgsparkl_amd import _ffi, models, solver

DIMS = (2, 3)
HDR = abi.header()
RUST = abi.read(abi.RUST_PATH)
HPP = abi.read(abi.HPP_PATH)

# header struct -> where its ctypes twin lives: an attribute of make_types(dim), a class of _ffi itself, or None — no binding code
# builds the record (instances are written by the device into caller memory, sample ids travel as a numpy array): size alone.
CTYPES_TWIN = {
    "wgs_sim_params": "T.SimParams", "wgs_elastic_coefficients": "T.Elastic", "wgs_drucker_prager": "T.DruckerPrager",
    "wgs_plastic_state": "T.PlasticState", "wgs_particle_phase": "T.Phase", "wgs_cdf": "T.Cdf", "wgs_particle_dynamics": "T.Dynamics",
    "wgs_particle": "T.Particle", "wgs_pose": "T.Pose", "wgs_velocity": "T.Velocity", "wgs_collider": "T.Collider",
    "wgs_mass_properties": "T.MassProperties", "wgs_node_record": "T.NodeRecord", "wgs_block_record": "T.BlockRecord",
    "wgs_stats": "T.Stats", "wgs_grid_sample": "T.GridSample", "wgs_particle_field": "T.ParticleField",
    "wgs_device_ptrs": "_ffi.DevicePtrs", "wgs_wall": "_ffi.Wall", "wgs_fixed_sum": "_ffi.FixedSum", "wgs_diagnostics": "_ffi.Diagnostics",
    "wgs_sample_ids": None, "wgs_instance": None,
}
# size of a struct (field None) / offset of a field in bytes as (2D, 3D), written down once beside the derived comparison: what the reference's repr(C)
# records and this header's own comments ("12 bytes", "16 words in 3D, 10 in 2D", "14 words in 3D, 8 in 2D") say.
EXPECTED_BYTES = {
    ("wgs_particle", None): (132, 188), ("wgs_particle", "dynamics"): (8, 12), ("wgs_cdf", None): (24, 32),
    ("wgs_sim_params", None): (12, 16), ("wgs_collider", None): (88, 88), ("wgs_node_record", None): (32, 40),
    ("wgs_block_record", None): (16, 20), ("wgs_particle_field", None): (40, 64), ("wgs_grid_sample", None): (4 * 8, 4 * 14),
    ("wgs_wall", None): (12, 12), ("wgs_wall", "type"): (0, 0), ("wgs_wall", "friction"): (4, 4), ("wgs_wall", "plane"): (8, 8),
    ("wgs_instance", None): (96, 96), ("wgs_sample_ids", None): (16, 16),
}
# Python object -> the header constant it mirrors
PY_CONSTANTS = [
    (_ffi.WGS_OK, "WGS_OK"), (_ffi.ERR_INVALID_ARGUMENT, "WGS_ERR_INVALID_ARGUMENT"), (_ffi.ERR_NO_DEVICE, "WGS_ERR_NO_DEVICE"),
    (_ffi.ERR_HIP, "WGS_ERR_HIP"), (_ffi.ERR_GRID_OVERFLOW, "WGS_ERR_GRID_OVERFLOW"), (_ffi.ERR_KEY_RANGE, "WGS_ERR_KEY_RANGE"),
    (_ffi.ERR_UNSUPPORTED, "WGS_ERR_UNSUPPORTED"), (_ffi.ABI_VERSION, "WGS_ABI_VERSION"), (_ffi.WGS_NUM_PASSES, "WGS_NUM_PASSES"),
    (len(_ffi.PASS_NAMES), "WGS_NUM_PASSES"), (_ffi.NUM_SUMS, "WGS_NUM_SUMS"),
    *((v, "WGS_SUM_" + k.upper()) for k, v in _ffi.SUM_INDEX.items()),
    *((getattr(_ffi, "DIAG_" + k), "WGS_DIAG_" + k) for k in ("PARTICLES", "ENERGY", "GRID", "DIGEST")),
    *((getattr(m, "WALL_" + k), "WGS_WALL_" + k) for m in (_ffi, models) for k in ("NONE", "STICKY", "SLIP", "SEPARATE")),
    *((getattr(models, "MODEL_" + k), "WGS_MODEL_" + k) for k in ("COROTATED", "NEO_HOOKEAN", "FLUID", "PER_PARTICLE")),
    *((getattr(models, "PLASTICITY_" + k), "WGS_PLASTICITY_" + k) for k in ("DRUCKER_PRAGER", "SNOW")),
    *((getattr(solver, "SHAPE_" + k), "WGS_SHAPE_" + k) for k in ("BALL", "CUBOID", "CAPSULE", "MESH")),
]
RUST_OPAQUE = {"wgs_pipeline", "wgs_data", "wgs_comm"}           # handles: never a layout
RUST_CONST_NAME = {"WGS_ABI_VERSION": "ABI_VERSION"}
# no struct or prototype takes its length from it (wgs_velocity.angular has three slots in both dimensions); a const that depends on a
# cargo feature would be the one line of the file the layout model cannot evaluate
RUST_NOT_MIRRORED = {"WGS_ANG_DIM"}
# entry points include/wgsparkl_hip.hpp does not wrap (today's 25): a new entry point is either wrapped or consciously listed here
CPP_NOT_WRAPPED = {
    "wgs_dim", "wgs_build_info", "wgs_set_rigid_particles", "wgs_prep_vertex_buffer", "wgs_prep_vertex_buffer_device",
    "wgs_set_plastic_state", "wgs_read_grid", "wgs_read_blocks", "wgs_read_timing_overhead", "wgs_set_uniform_material",
    "wgs_set_grid_growth", "wgs_debug_scan", "wgs_data_create_sharded", "wgs_shard_halo_record_bytes",
    "wgs_shard_particle_record_bytes", "wgs_shard_buffer_header_bytes", "wgs_set_stream", "wgs_shard_export", "wgs_comm_get_unique_id",
    "wgs_comm_create", "wgs_comm_destroy", "wgs_shard_attach", "wgs_sharded_step", "wgs_sharded_step_lockstep", "wgs_enqueue_diagnostics",
}


# ------------------------------------------------------------------------------------------------ the comparisons
def ctypes_twins(dim):
    T = _ffi.make_types(dim)
    return {s: getattr(T if where.startswith("T.") else _ffi, where.split(".")[1]) for s, where in CTYPES_TWIN.items() if where}


def ctypes_struct_problems(hdr, lay, twins, no_twin=()):
    bad = [f"{s}: no ctypes twin" for s in hdr.structs if s not in twins and s not in no_twin]
    for s, ct in twins.items():
        if s not in lay.size:
            continue
        if C.sizeof(ct) != lay.size[s]:
            bad.append(f"{s}: ctypes {C.sizeof(ct)} bytes, header {lay.size[s]}")
        if len(ct._fields_) != len(hdr.structs[s]):
            bad.append(f"{s}: ctypes {len(ct._fields_)} fields, header {len(hdr.structs[s])}")
        for f, want in lay.fields[s].items():
            d = getattr(ct, f, None) or getattr(ct, f + "_", None)           # `lambda_` stands for `lambda`
            got = (d.offset, d.size) if d is not None else None
            if got != want:
                bad.append(f"{s}.{f}: ctypes (offset, size) {got}, header {want}")
    return bad


def ctypes_prototype_problems(hdr, protos):
    if list(protos) != list(hdr.functions):
        return [f"names or order: only ctypes {[n for n in protos if n not in hdr.functions]}, only header "
                f"{[n for n in hdr.functions if n not in protos]}, else the order differs"]
    lp64 = lambda kinds: ["size" if k == "u64" else k for k in kinds]       # (abi.ctypes_kind: one ctypes class for both)
    bad = []
    for name, (ret, params) in hdr.functions.items():
        restype, argtypes = protos[name]
        got = (abi.ctypes_kind(restype), [abi.ctypes_kind(t) for t in argtypes])
        want = (abi.return_kind(ret), lp64(abi.param_kinds(params)))
        if got != want:
            bad.append(f"{name}: ctypes {got}, header {want}")
    return bad


def rust_struct_problems(hdr, lay, rust):
    bad = [f"{s}: not declared in lib.rs" for s in hdr.structs if s not in rust.size]
    bad += [f"{s}: declared in lib.rs, not in the header" for s in rust.size if s not in hdr.structs and s not in RUST_OPAQUE]
    for s in hdr.structs:
        if s in rust.size and s in lay.size and (rust.size[s], rust.fields[s]) != (lay.size[s], lay.fields[s]):
            bad.append(f"{s}: lib.rs {rust.size[s]} {rust.fields[s]}, header {lay.size[s]} {lay.fields[s]}")
    return bad


def rust_constant_problems(hdr, lay, rust):
    bad = []
    for c in hdr.constants:
        name = RUST_CONST_NAME.get(c, c)
        if c in RUST_NOT_MIRRORED:
            if name in rust.const:
                bad.append(f"{c}: listed as not mirrored, yet declared")
        elif name not in rust.const:
            bad.append(f"{c}: not declared in lib.rs")
        elif c in lay.const and rust.const[name] != lay.const[c]:
            bad.append(f"{c}: lib.rs {rust.const[name]}, header {lay.const[c]}")
    return bad


def rust_function_problems(hdr, fns):
    bad = [f"{n}: not in the extern block" for n in hdr.functions if n not in fns]
    bad += [f"{n}: in the extern block, not in the header" for n in fns if n not in hdr.functions]
    for name, (ret, params) in hdr.functions.items():
        want = (abi.return_kind(ret), abi.param_kinds(params))
        if name in fns and fns[name] != want:
            bad.append(f"{name}: lib.rs {fns[name]}, header {want}")
    return bad


def cpp_problems(hdr, hpp):
    wrapped = {n for n in hdr.functions if n + "(" in hpp}
    return ([f"{n}: neither wrapped by wgsparkl_hip.hpp nor listed" for n in hdr.functions if n not in wrapped | CPP_NOT_WRAPPED] +
            [f"{n}: listed as not wrapped, yet the wrapper calls it" for n in sorted(wrapped & CPP_NOT_WRAPPED)] +
            [f"{n}: listed as not wrapped, not in the header" for n in sorted(CPP_NOT_WRAPPED - set(hdr.functions))])


# ------------------------------------------------------------------------------------------------ the header itself
def test_the_table_is_the_whole_header():
    assert (len(HDR.structs), sum(map(len, HDR.structs.values())), len(HDR.constants), len(HDR.functions)) == (23, 112, 59, 58)
    assert set(CTYPES_TWIN) == set(HDR.structs), "the twin map names every struct, and nothing else"
    for dim in DIMS:
        lay = abi.layout(dim)
        assert set(lay.size) == set(HDR.structs) and set(lay.const) == set(HDR.constants)
        assert {s: list(fs) for s, fs in lay.fields.items()} == HDR.structs
        assert lay.const["WGS_ANG_DIM"] == (1, 3)[dim - 2]


@pytest.mark.parametrize("dim", DIMS)
def test_sizes_written_down_once(dim):
    lay = abi.layout(dim)
    for (s, f), want in EXPECTED_BYTES.items():
        assert (lay.size[s] if f is None else lay.fields[s][f][0]) == want[dim - 2], (s, f)
    # wgs_particle is the repr(C) image of Particle (particle3d.rs:53-60): all 4-byte members, no padding
    assert lay.size["wgs_particle"] == 4 * (dim + (dim + 2 * dim * dim + 2 * dim + 2 + 3) + 2 + 1 + 6 + 1 + 2)


def test_abi_version_is_seven_and_the_header_says_how_to_detect_what_came_since():
    """The one place that spells the number. Everything added at 7 touched no struct, enum value or signature that existed; the history
    paragraph names, per feature, the symbol a binding looks up on an older library of the same version."""
    assert {abi.layout(dim).const["WGS_ABI_VERSION"] for dim in DIMS} == {_ffi.ABI_VERSION} and _ffi.ABI_VERSION == 7
    text = " ".join(abi.read(abi.HEADER_PATH).replace("\n *", " ").split())
    history = text[text.index("History: 5 ="):text.index("#define WGS_ABI_VERSION")]
    for symbol in ("wgs_set_fluid_eos", "wgs_set_particle_models", "wgs_sample_grid", "wgs_read_particle_fields", "wgs_set_domain_walls",
                   "wgs_set_plasticity_model"):
        assert re.search(rf"detects? {symbol} by symbol lookup", history), symbol
    assert history.count("Still 7:") == 6


# ------------------------------------------------------------------------------------------------ ctypes
@pytest.mark.parametrize("dim", DIMS)
def test_every_struct_has_a_ctypes_twin_of_the_same_layout(dim):
    size_only = {s for s, where in CTYPES_TWIN.items() if where is None}
    assert size_only == {"wgs_instance", "wgs_sample_ids"}
    assert ctypes_struct_problems(HDR, abi.layout(dim), ctypes_twins(dim), size_only) == []


@pytest.mark.parametrize("dim", DIMS)
def test_ctypes_prototypes_are_the_headers(dim):
    """Exactly the header's functions in the header's order, the declared return type, and every parameter of the declared kind:
    nothing is left to ctypes' defaults."""
    protos = _ffi.prototypes(_ffi.make_types(dim))
    assert ctypes_prototype_problems(HDR, protos) == []
    assert list(_ffi.EXPORTS) == list(HDR.functions)


@pytest.mark.parametrize("dim", DIMS)
def test_library_exports_every_declared_symbol(hip_libs, dim):
    """... and the functions of the loaded library carry those prototypes, not ctypes' defaults."""
    lib, _ = hip_libs.load(dim)
    for name in HDR.functions:
        assert hasattr(lib, name), f"libwgsparkl{dim}d_hip.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, f"{name}: no argtypes"
    assert ctypes_prototype_problems(HDR, {n: (getattr(lib, n).restype, getattr(lib, n).argtypes) for n in HDR.functions}) == []
    assert lib.wgs_dim() == dim
    assert lib.wgs_abi_version() == abi.layout(dim).const["WGS_ABI_VERSION"]


def test_python_constants_are_the_headers():
    for dim in DIMS:
        const = abi.layout(dim).const
        for value, name in PY_CONSTANTS:
            assert value == const[name], name
    mirrored = {name for _, name in PY_CONSTANTS}
    for family in ("WGS_ERR_", "WGS_SUM_", "WGS_DIAG_", "WGS_WALL_", "WGS_MODEL_", "WGS_PLASTICITY_", "WGS_SHAPE_"):
        assert {c for c in HDR.constants if c.startswith(family)} <= mirrored, family
    assert _ffi.DIAG_ALL == sum(v for c, v in abi.layout(3).const.items() if c.startswith("WGS_DIAG_"))


# ------------------------------------------------------------------------------------------------ Rust
@pytest.mark.parametrize("dim", DIMS)
def test_rust_structs_and_constants_are_the_headers(dim):
    lay, rust = abi.layout(dim), abi.rust_layout(RUST, dim)
    assert rust_struct_problems(HDR, lay, rust) == []
    assert rust_constant_problems(HDR, lay, rust) == []


def test_rust_extern_block_is_the_headers():
    assert rust_function_problems(HDR, abi.rust_functions(RUST)) == []
    # the version check the header asks of every binding exists in the crate and INTEGRATION.md §2 points at it
    assert re.search(r"pub fn check_abi\(\) -> Result<\(\), u32>", RUST) and "wgs_abi_version()" in RUST.split("pub fn check_abi")[1].split("extern")[0]
    assert "check_abi()" in abi.read(os.path.join(abi.ROOT, "INTEGRATION.md"))


# ------------------------------------------------------------------------------------------------ C++
def test_cpp_wrapper_wraps_every_entry_point_or_it_is_listed():
    assert cpp_problems(HDR, HPP) == []
    assert len(CPP_NOT_WRAPPED) == 25


# ------------------------------------------------------------------------------------------------ the checks can fail
def _swap(text, a, b):
    assert a in text and b in text
    return text.replace(a, "\0").replace(b, a).replace("\0", b)


def test_rust_layout_model_sees_a_wrong_struct():
    swapped = _swap(RUST, "pub grid_growths: u32,", "pub cell_changers: u64,")
    short = RUST.replace("pub angular: [f32; 3],", "pub angular: [f32; DIM],")
    gone = re.sub(r"#\[repr\(C\)\]\s*#\[derive\(Copy, Clone\)\]\s*pub struct wgs_pose \{[^}]*\}", "", RUST)
    assert swapped != RUST and short != RUST and gone != RUST
    for dim in DIMS:
        lay = abi.layout(dim)
        bad = rust_struct_problems(HDR, lay, abi.rust_layout(swapped, dim))
        assert len(bad) == 1 and bad[0].startswith("wgs_stats:"), bad
        # an array sized by DIM where the header says 3: right by accident in 3D — why both dimensions are always compared
        bad = rust_struct_problems(HDR, lay, abi.rust_layout(short, dim))
        assert [b.split(":")[0] for b in bad] == ([] if dim == 3 else ["wgs_velocity", "wgs_collider"]), bad
    with pytest.raises(AssertionError, match="wgs_pose"):                     # (wgs_collider nests it: the file no longer stands)
        abi.rust_layout(gone, 3)
    leaf = re.sub(r"#\[repr\(C\)\]\s*#\[derive\(Copy, Clone\)\]\s*pub struct wgs_wall \{[^}]*\}", "", RUST)
    assert rust_struct_problems(HDR, abi.layout(3), abi.rust_layout(leaf, 3)) == ["wgs_wall: not declared in lib.rs"]


def test_rust_constant_and_parameter_checks_see_a_wrong_one():
    lay = abi.layout(3)
    gone = RUST.replace("pub const WGS_ERR_KEY_RANGE: wgs_status = 5;\n", "")
    other = RUST.replace("pub const WGS_SUM_ANGULAR: usize = 4;", "pub const WGS_SUM_ANGULAR: usize = 3;")
    assert gone != RUST and other != RUST
    assert rust_constant_problems(HDR, lay, abi.rust_layout(gone, 3)) == ["WGS_ERR_KEY_RANGE: not declared in lib.rs"]
    assert rust_constant_problems(HDR, lay, abi.rust_layout(other, 3)) == ["WGS_SUM_ANGULAR: lib.rs 3, header 4"]
    narrow = RUST.replace("points: *const f32, n: usize, out: *mut wgs_grid_sample", "points: *const f32, n: u32, out: *mut wgs_grid_sample")
    assert narrow != RUST
    bad = rust_function_problems(HDR, abi.rust_functions(narrow))
    assert len(bad) == 1 and bad[0].startswith("wgs_sample_grid:"), bad


def test_ctypes_checks_see_a_wrong_struct_and_a_wrong_prototype():
    lay, twins = abi.layout(3), ctypes_twins(3)

    class Dropped(C.Structure):
        _fields_ = _ffi.Wall._fields_[:2]

    class Wide(C.Structure):
        _fields_ = [("type", C.c_uint64)] + _ffi.Wall._fields_[1:]

    for wrong, said in ((Dropped, "wgs_wall.plane"), (Wide, "wgs_wall.type")):
        bad = ctypes_struct_problems(HDR, lay, {**twins, "wgs_wall": wrong}, {"wgs_instance", "wgs_sample_ids"})
        assert bad and all(b.startswith("wgs_wall") for b in bad) and any(b.startswith(said) for b in bad), bad
    protos = dict(_ffi.prototypes(_ffi.make_types(3)))
    restype, argtypes = protos["wgs_get_stats"]
    protos["wgs_get_stats"] = (restype, [argtypes[0], C.c_uint32])
    bad = ctypes_prototype_problems(HDR, protos)
    assert len(bad) == 1 and bad[0].startswith("wgs_get_stats:"), bad
    del protos["wgs_get_stats"]
    assert ctypes_prototype_problems(HDR, protos)


def test_a_struct_a_constant_and_a_function_without_mirrors_are_named_by_every_check():
    """The header grows by one of each in a copy; nothing else changes. Every mirror check must miss exactly the newcomers."""
    text = abi.read(abi.HEADER_PATH).replace(
        "#define WGS_ABI_VERSION 7",
        "#define WGS_ABI_VERSION 7\ntypedef struct { float a, b[2]; } wgs_newcomer;\n#define WGS_NEW_LIMIT 4\n"
        "wgs_status wgs_new_call(wgs_data *data, const wgs_newcomer *in);")
    grown = abi.header(text)
    assert grown.structs["wgs_newcomer"] == ["a", "b"] and "WGS_NEW_LIMIT" in grown.constants and "wgs_new_call" in grown.functions
    lay = abi.layout(3)                                  # (of the real header: the newcomers are reported before a layout is asked for)
    assert ctypes_struct_problems(grown, lay, ctypes_twins(3), {"wgs_instance", "wgs_sample_ids"}) == ["wgs_newcomer: no ctypes twin"]
    assert len(ctypes_prototype_problems(grown, _ffi.prototypes(_ffi.make_types(3)))) == 1
    rust = abi.rust_layout(RUST, 3)
    assert rust_struct_problems(grown, lay, rust) == ["wgs_newcomer: not declared in lib.rs"]
    assert rust_constant_problems(grown, lay, rust) == ["WGS_NEW_LIMIT: not declared in lib.rs"]
    assert rust_function_problems(grown, abi.rust_functions(RUST)) == ["wgs_new_call: not in the extern block"]
    assert cpp_problems(grown, HPP) == ["wgs_new_call: neither wrapped by wgsparkl_hip.hpp nor listed"]
    # ... and the newest entry point of the real header, taken out of a copy of each mirror, is named by that mirror's check
    gone = "wgs_get_plasticity_model"
    protos = {n: p for n, p in _ffi.prototypes(_ffi.make_types(3)).items() if n != gone}
    bad = ctypes_prototype_problems(HDR, protos)
    assert len(bad) == 1 and f"only header ['{gone}']" in bad[0], bad
    less = RUST.replace(f"    pub fn {gone}(d: *mut wgs_data, out: *mut i32) -> wgs_status;\n", "")
    assert less != RUST and rust_function_problems(HDR, abi.rust_functions(less)) == [f"{gone}: not in the extern block"]
    less = HPP.replace(gone + "(", "(")
    assert less != HPP and cpp_problems(HDR, less) == [f"{gone}: neither wrapped by wgsparkl_hip.hpp nor listed"]
