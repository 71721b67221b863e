"""-m "not gpu": the particle-removal extension (include/wgsparkl_hip_remove.h) as far as a box without a GPU sees it, the way
tests/test_emit_abi.py holds the run-time particle extension: the struct's layout from a compiled C probe through the main header alone,
both dimensions; the declarations and the rule's sentences; the include order and the build's hash list; the ctypes twin and prototypes;
the Rust file against the extension header with tests/abi.py's parser; the C++ wrappers; NULL-argument statuses; models.Sink's
validation; the scene key and the two scenes, sized on the CPU with emit_truth and remove_truth. No compute call is made."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi

EXT_PATH = os.path.join(abi.INCLUDE, "wgsparkl_hip_remove.h")
RUST_PATH = os.path.join(abi.ROOT, "rust", "wgsparkl-hip-sys", "src", "remove.rs")
EXT = abi.header(abi.read(EXT_PATH))
FIELDS = ["region", "side", "center", "half", "start_substep", "period"]
CONSTANTS = {"WGS_SINK_INSIDE": 0, "WGS_SINK_OUTSIDE": 1, "WGS_MAX_SINKS": 8}
FUNCTIONS = ["wgs_remove_particles", "wgs_remove_particles_device", "wgs_remove_particles_in", "wgs_set_sinks", "wgs_get_sinks",
             "wgs_get_sink_counts", "wgs_debug_compact_map"]
SIZE = 40
OFFSETS = {"region": (0, 4), "side": (4, 4), "center": (8, 12), "half": (20, 12), "start_substep": (32, 4), "period": (36, 4)}


def test_the_extension_header_declares_exactly_the_feature():
    assert EXT.structs == {"wgs_sink": FIELDS}
    assert EXT.constants == list(CONSTANTS) and list(EXT.functions) == FUNCTIONS
    text = abi.read(EXT_PATH)
    for line in ("#define WGS_MAX_SINKS 8", "enum { WGS_SINK_INSIDE = 0, WGS_SINK_OUTSIDE = 1 };",
                 "WGS_REGION_BOX   inside  <=>  fabsf(d_k) <= half_k on every axis k < WGS_DIM;",
                 "WGS_REGION_BALL  inside  <=>  s <= fl(half_0 * half_0), s = fl(d_0 * d_0); s = fl(s + fl(d_1 * d_1)); [3D: s = fl(s + fl(d_2 * d_2));]",
                 "d_k = fl(x_k - center_k), k < WGS_DIM, every fl() a rounding of its own (no contraction)",
                 "s >= start_substep  and  (s - start_substep) % period == 0.",
                 "wgs_status wgs_remove_particles(wgs_data *data, const uint8_t *remove, uint32_t *kept_from /* or NULL */, uint32_t *num_removed);",
                 "wgs_status wgs_get_sink_counts(wgs_data *data, uint64_t removed[WGS_MAX_SINKS]);"):
        assert line in text, line
    for said in ("refusals change nothing", "WGS_PASS_GRID_SORT", "wgs_stats.table_rebuilds", "the first of them in array order", "Blocking",
                 "not part of a checkpoint", "no device memory", "wgs_stats.device_bytes does not change", "On a face (==) counts as inside",
                 "A comparison with a NaN is false", "WGS_REGION_ALL is refused", "in front of the emitters of that substep", "ONE pass",
                 "its old index minus the number of removed particles in front of it", "kept_from is increasing", "the value wgs_read_positions answers",
                 "one stream synchronisation", "bit-identical to one without sinks", "Removing every particle is allowed",
                 "Not part of this extension: removal on sharded data; removal without a table rebuild; sinks that need no synchronisation"):
        assert said in " ".join(text.replace("\n *", " ").split()), said
    main = abi.read(abi.HEADER_PATH)
    flat = " ".join(main.replace("\n *", " ").split())
    assert ("and, still 7, the particle-removal extension of wgsparkl_hip_remove.h (masks, regions, scheduled sinks) — detect "
            "wgs_remove_particles by symbol lookup") in flat
    assert "#define WGS_ABI_VERSION 7" in main
    assert main.index('#include "wgsparkl_hip_emit.h"') < main.index('#include "wgsparkl_hip_remove.h"') < main.index("wgs_debug_scan(")
    hdr = abi.header()
    assert "wgs_sink" not in hdr.structs and not set(CONSTANTS) & set(hdr.constants) and not set(FUNCTIONS) & set(hdr.functions)
    emit = abi.read(os.path.join(abi.INCLUDE, "wgsparkl_hip_emit.h"))
    assert "Removing particles (sinks, outflow) and appending without a rebuild are not part of this extension." in " ".join(emit.replace("\n *", " ").split())
    build = abi.read(os.path.join(abi.ROOT, "wgsparkl_amd", "csrc", "build.sh"))
    assert "../../include/wgsparkl_hip_remove.h" in build.split("sources=")[1].splitlines()[0], "a changed extension header must rebuild the libraries"
    capi = abi.read(os.path.join(abi.ROOT, "wgsparkl_amd", "csrc", "capi.hip"))
    assert capi.index('#include "capi_emit.inc"') < capi.index('#include "kernels_remove.h"') < capi.index('#include "capi_remove.inc"')
    assert capi.rstrip().splitlines()[-1].startswith('#include "capi_remove.inc"'), "included last: no kernel that existed changes its place"


@pytest.mark.parametrize("dim", [2, 3])
def test_struct_layout_from_a_compiled_probe_through_the_main_header_alone(dim, tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "wgsparkl_hip.h"', "int main(void) {",
             '  printf("S %zu\\n", sizeof(wgs_sink));']
    lines += [f'  printf("F {f} %zu %zu\\n", offsetof(wgs_sink, {f}), sizeof(((wgs_sink *)0)->{f}));' for f in FIELDS]
    lines += [f'  printf("C {c} %d\\n", (int){c});' for c in CONSTANTS]
    lines += ['  printf("R %d %d\\n", (int)WGS_REGION_BOX, (int)WGS_REGION_BALL);']
    lines += ["  return wgs_remove_particles == NULL || wgs_set_sinks == NULL || wgs_debug_compact_map == NULL;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    # (compiled, not linked against the library: the addresses are taken in a translation unit of their own)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-address", f"-DWGS_DIM={dim}", f"-I{abi.INCLUDE}", "-c", str(src), "-o", str(tmp_path / "probe.o")], check=True)
    src.write_text("\n".join(lines).replace("return wgs_remove_particles == NULL || wgs_set_sinks == NULL || wgs_debug_compact_map == NULL;", "return 0;") + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-DWGS_DIM={dim}", f"-I{abi.INCLUDE}", str(src), "-o", str(exe)], check=True)
    out = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert ["S", str(SIZE)] in out and ["R", "1", "2"] in out
    assert {l[1]: int(l[2]) for l in out if l[0] == "C"} == CONSTANTS
    assert {l[1]: (int(l[2]), int(l[3])) for l in out if l[0] == "F"} == OFFSETS


def test_ctypes_twin_and_prototypes():
    from wgsparkl_amd import _ffi, models
    ct = _ffi.Sink
    assert C.sizeof(ct) == SIZE and [f for f, _ in ct._fields_] == FIELDS
    assert {f: (getattr(ct, f).offset, getattr(ct, f).size) for f in FIELDS} == OFFSETS
    protos = _ffi.remove_prototypes()
    assert list(protos) == list(EXT.functions)
    for name, (ret, params) in EXT.functions.items():
        restype, argtypes = protos[name]
        assert (abi.ctypes_kind(restype), [abi.ctypes_kind(t) for t in argtypes]) == (abi.return_kind(ret), abi.param_kinds(params)), name
    for dim in (2, 3):
        T = _ffi.make_types(dim)
        others = {**_ffi.prototypes(T), **_ffi.forces_prototypes(), **_ffi.emit_prototypes(T, dim)}
        assert not set(protos) & set(others) and not set(protos) & set(_ffi.EXPORTS)
    assert _ffi.MAX_SINKS == models.MAX_SINKS == 8
    assert (_ffi.SINK_INSIDE, _ffi.SINK_OUTSIDE) == (models.SINK_INSIDE, models.SINK_OUTSIDE) == (0, 1)
    assert (models.REGION_BOX, models.REGION_BALL) == (_ffi.REGION_BOX, _ffi.REGION_BALL) == (1, 2)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_loaded_library_carries_the_prototypes(hip_libs, dim):
    lib, T = hip_libs.load(dim)
    for name, (restype, argtypes) in hip_libs.remove_prototypes().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_rust_file_is_the_extension_headers():
    text = abi.read(RUST_PATH)
    for dim in (2, 3):
        rust = abi.rust_layout(text, dim)
        assert rust.size["wgs_sink"] == SIZE and rust.fields["wgs_sink"] == OFFSETS
        assert rust.const == {"WGS_MAX_SINKS": 8, "WGS_SINK_INSIDE": 0, "WGS_SINK_OUTSIDE": 1}
    fns = abi.rust_functions(text)
    assert list(fns) == list(EXT.functions)
    for name, (ret, params) in EXT.functions.items():
        assert fns[name] == (abi.return_kind(ret), abi.param_kinds(params)), name
    lib_rs = abi.read(abi.RUST_PATH)
    assert "pub mod remove;" in lib_rs and "wgs_sink" not in lib_rs and lib_rs.index("pub mod emit;") < lib_rs.index("pub mod remove;")


def test_cpp_wrapper_wraps_them_all():
    hpp = abi.read(abi.HPP_PATH)
    for name in EXT.functions:
        if name not in ("wgs_debug_compact_map", "wgs_remove_particles_device"):       # (a test hook; the device form takes raw pointers)
            assert name + "(" in hpp, name
    for said in ("std::vector<uint32_t> remove_particles(const std::vector<uint8_t> &remove)",
                 "std::vector<uint32_t> remove_particles_in(const std::vector<wgs_sink> &regions)",
                 "void set_sinks(const std::vector<wgs_sink> &sinks)", "std::vector<wgs_sink> sinks()", "std::vector<uint64_t> sink_counts() const",
                 "for (uint64_t r : sink_counts()) n -= (size_t)r;"):
        assert said in hpp, said


@pytest.mark.parametrize("dim", [2, 3])
def test_calls_without_a_handle_fail_through_the_status_path(hip_libs, dim):
    """No wgs_data can be created without a GPU: a NULL handle is WGS_ERR_INVALID_ARGUMENT with a message, and nothing is written."""
    lib, T = hip_libs.load(dim)
    arr = (hip_libs.Sink * hip_libs.MAX_SINKS)()
    C.memset(arr, 0x5a, C.sizeof(arr))
    n, removed = C.c_uint32(0x5a5a5a5a), C.c_uint32(0x5a5a5a5a)
    counts = (C.c_uint64 * 8)(*([7] * 8))
    mask, kept = (C.c_uint8 * 4)(1, 0, 1, 0), (C.c_uint32 * 4)(9, 9, 9, 9)
    for call in (lambda: lib.wgs_remove_particles(None, mask, kept, C.byref(removed)), lambda: lib.wgs_remove_particles_device(None, C.c_void_p(16), None, C.byref(removed)),
                 lambda: lib.wgs_remove_particles_in(None, arr, 1, kept, C.byref(removed)), lambda: lib.wgs_set_sinks(None, arr, 1),
                 lambda: lib.wgs_set_sinks(None, None, 0), lambda: lib.wgs_get_sinks(None, arr, C.byref(n)), lambda: lib.wgs_get_sink_counts(None, counts),
                 lambda: lib.wgs_debug_compact_map(None, mask, 4, kept, C.byref(n))):
        assert call() == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(arr) == b"\x5a" * C.sizeof(arr) and n.value == removed.value == 0x5a5a5a5a and list(counts) == [7] * 8 and list(kept) == [9] * 4


def test_sink_validation_and_the_helpers():
    from wgsparkl_amd.models import REGION_BALL, REGION_BOX, SINK_INSIDE, SINK_OUTSIDE, Sink
    from wgsparkl_amd.pipeline import MpmData
    for m in ("remove_particles", "remove_particles_device", "remove_particles_in", "set_sinks", "sinks", "sink_counts"):
        assert callable(getattr(MpmData, m))
    assert isinstance(MpmData.n, property)
    b = Sink.box((1.0, 2.0), (0.5, 0.25), start_substep=3, period=4)
    assert (b.region, b.side, b.center, b.half, b.start_substep, b.period) == (REGION_BOX, SINK_INSIDE, (1.0, 2.0, 0.0), (0.5, 0.25, 0.0), 3, 4)
    r = Sink.ball((1.0, 2.0, 3.0), 1.5)
    assert (r.region, r.side, r.half, r.period, r.start_substep) == (REGION_BALL, SINK_INSIDE, (1.5, 0.0, 0.0), 1, 0)
    o = Sink.outside_box((1.0, 2.0, 3.0), (4.0, 5.0, 6.0), period=2)
    assert (o.region, o.side, o.half, o.period) == (REGION_BOX, SINK_OUTSIDE, (4.0, 5.0, 6.0), 2)
    bad = [dict(region=0), dict(region=3), dict(side=2), dict(period=0), dict(period=1.5), dict(period=2 ** 32), dict(start_substep=-1),
           dict(start_substep=2 ** 32), dict(center=(0.0, float("nan"), 0.0)), dict(center=(0.0, 0.0)), dict(half=(1.0, -1.0, 1.0)),
           dict(half=(float("inf"), 1.0, 1.0)), dict(half=(1.0, 1.0))]
    for kw in bad:
        args = dict(region=REGION_BOX, side=SINK_INSIDE, center=(0.0, 0.0, 0.0), half=(1.0, 1.0, 1.0))
        args.update(kw)
        with pytest.raises(ValueError):
            Sink(**args)


def _free_flight(pos, vel, gravity, dt, substeps):
    """v += g dt, x += v dt, in fp64"""
    x, v = np.asarray(pos, np.float64).copy(), np.broadcast_to(np.asarray(vel, np.float64), np.shape(pos)).copy()
    for _ in range(substeps):
        v += np.asarray(gravity, np.float64) * dt
        x += v * dt
    return x


def test_scene_key_the_new_scenes_and_the_documents():
    import emit_truth as ET
    import remove_truth as RT
    from wgsparkl_amd import scenes
    from wgsparkl_amd.models import MODEL_FLUID, SINK_INSIDE, SINK_OUTSIDE
    from wgsparkl_amd.sharded import NativeShard
    doc = scenes.__doc__
    assert "| `sinks` |" in doc and doc.index("| `emitters` |") < doc.index("| `sinks` |")
    for dim in (2, 3):
        for make, side in ((scenes.drain, SINK_INSIDE), (scenes.channel, SINK_OUTSIDE)):
            sc = make(dim)
            em, sink, params = sc["emitters"][0], sc["sinks"][0], sc["params"]
            assert sc["particles"].n == 0 and sc["model"] == MODEL_FLUID and len(sc["sinks"]) == 1 and sink.side == side and em.batches == 0
            transit = sc["transit_substeps"]
            # by construction, not by luck: in free flight every particle of a batch is still there just after it was emitted, has been
            # taken by the sink's region `transit` substeps later, and stays taken for a sink period more
            for q in (0, 3):
                pos = ET.batch_positions(em, 0, q)
                assert not RT.takes(sink, pos).any()
                for k in range(transit, transit + sink.period + 1):
                    assert RT.takes(sink, _free_flight(pos, em.proto.vel[0], params.gravity, params.dt, k).astype(np.float32)).all(), (dim, k)
            # ... so at most ceil((transit + sink period) / emitter period) + 1 batches are alive, and the capacity is twice that
            alive = (-(-(transit + sink.period) // em.period) + 1) * em.batch_size
            assert sc["particle_capacity"] == 2 * alive and em.batch_size <= alive
            worst, born = 0, []
            for s in range(3 * transit):                       # the schedules, played on the CPU under free flight
                if RT.due(sink, s):
                    born = [b for b in born if s - b < transit]
                if ET.due(em, s) is not None:
                    born.append(s)
                worst = max(worst, len(born) * em.batch_size)
            assert 0 < worst <= alive
            # a slab refuses the key before it touches the library
            with pytest.raises(ValueError, match="sinks"):
                NativeShard.from_scene(None, {k: v for k, v in sc.items() if k not in ("emitters", "particle_capacity", "walls")}, 0)
    for make in (scenes.dam_break, scenes.block_in_fluid, scenes.walled_box, scenes.snowball, scenes.vortex_tank, scenes.faucet, scenes.sand_pour,
                 scenes.reference_smoke_scene, lambda: scenes.neo_hookean_cube(n_side=4), lambda: scenes.sand_column(4, 4, 4)):
        assert "sinks" not in make()
    for doc, said in (("INTEGRATION.md", "wgs_remove_particles"), ("INTEGRATION.md", "wgs_set_sinks"), ("README.md", "wgs_remove_particles"),
                      ("DESIGN.md", "## 7g. Particles removed at run time"), ("DESIGN.md", "k_remove_compact"), ("tools/README.md", "gpu_remove_prof.py"),
                      ("notes/round_35.md", "kernel_symbols_cmp")):
        assert said in abi.read(os.path.join(abi.ROOT, doc)), (doc, said)
