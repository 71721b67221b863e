"""-m "not gpu": the run-time particle extension (include/wgsparkl_hip_emit.h) as far as a box without a GPU sees it, the way
tests/test_force_abi.py holds the force-field extension: the struct's layout from a compiled C probe through the main header alone, both
dimensions; the declarations and the rule's sentences; the ctypes twin and prototypes; the Rust file against the extension header with
tests/abi.py's parser; the C++ wrappers; NULL-argument statuses; models.Emitter's validation; the scene keys. No compute call is made."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import abi

EXT_PATH = os.path.join(abi.INCLUDE, "wgsparkl_hip_emit.h")
RUST_PATH = os.path.join(abi.ROOT, "rust", "wgsparkl-hip-sys", "src", "emit.rs")
EXT = abi.header(abi.read(EXT_PATH))
FIELDS = ["proto", "model", "lo", "count", "spacing", "jitter", "seed", "start_substep", "period", "batches"]
FUNCTIONS = ["wgs_data_create_reserved", "wgs_get_particle_capacity", "wgs_add_particles", "wgs_set_emitters", "wgs_get_emitters",
             "wgs_get_emitter_counts"]
SIZE = {2: 176, 3: 240}
PARTICLE = {2: 132, 3: 188}


def offsets(dim):
    """wgs_emitter by the C rules, written out: the particle, one byte and three of padding, then words"""
    p, d = PARTICLE[dim], 4 * dim
    at = {"proto": (0, p), "model": (p, 1), "lo": (p + 4, d), "count": (p + 4 + d, d)}
    for k, f in enumerate(FIELDS[4:]):
        at[f] = (p + 4 + 2 * d + 4 * k, 4)
    return at


def test_the_extension_header_declares_exactly_the_feature():
    assert EXT.structs == {"wgs_emitter": FIELDS}
    assert EXT.constants == ["WGS_MAX_EMITTERS"] and list(EXT.functions) == FUNCTIONS
    text = abi.read(EXT_PATH)
    for line in ("#define WGS_MAX_EMITTERS 8",
                 "x_k = fl(fl(lo_k + fl(fl((float)i_k + 0.5f) * spacing)) + fl(fl(jitter * spacing) * u_k))",
                 "u_k  = (float)(hash >> 8) * 2^-24 - 0.5f",
                 "hash = wgs_lowbias32(seed ^ wgs_lowbias32(q * 0x9E3779B9u + e) ^ wgs_lowbias32(point_index * WGS_DIM + k))",
                 "q = (s - start_substep) / period     if  s >= start_substep,  (s - start_substep) % period == 0  and  (q < batches or batches == 0).",
                 "x *= 0x7feb352dU;", "x *= 0x846ca68bU;",
                 "wgs_status wgs_add_particles(wgs_data *data, const wgs_particle *particles, const uint8_t *models /* k bytes or NULL */, size_t k);"):
        assert line in text, line
    for said in ("refusals change nothing", "WGS_PASS_GRID_SORT", "wgs_stats.table_rebuilds", "Emitters fire in array order", "skipped and counted",
                 "tried again", "x fastest", "Blocking", "not part of a checkpoint", "no device memory", "Removing particles"):
        assert said in " ".join(text.replace("\n *", " ").split()), said
    main = abi.read(abi.HEADER_PATH)
    flat = " ".join(main.replace("\n *", " ").split())
    assert "and, still 7, the run-time particle extension of wgsparkl_hip_emit.h (reserved capacity, appended batches, emitters) — detect wgs_add_particles by symbol lookup" in flat
    assert main.index('#include "wgsparkl_hip_forces.h"') < main.index('#include "wgsparkl_hip_emit.h"') < main.index("wgs_debug_scan(")
    hdr = abi.header()
    assert "wgs_emitter" not in hdr.structs and "WGS_MAX_EMITTERS" not in hdr.constants and not set(FUNCTIONS) & set(hdr.functions)
    build = abi.read(os.path.join(abi.ROOT, "wgsparkl_amd", "csrc", "build.sh"))
    assert "../../include/wgsparkl_hip_emit.h" in build.split("sources=")[1].splitlines()[0], "a changed extension header must rebuild the libraries"


@pytest.mark.parametrize("dim", [2, 3])
def test_struct_layout_and_the_mixer_from_a_compiled_probe_through_the_main_header_alone(dim, tmp_path):
    import emit_truth as ET
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "wgsparkl_hip.h"', "int main(void) {",
             '  printf("S %zu %zu\\n", sizeof(wgs_emitter), sizeof(wgs_particle));']
    lines += [f'  printf("F {f} %zu %zu\\n", offsetof(wgs_emitter, {f}), sizeof(((wgs_emitter *)0)->{f}));' for f in FIELDS]
    lines += ['  printf("C %d\\n", (int)WGS_MAX_EMITTERS);']
    lines += [f'  printf("H %u\\n", (unsigned)wgs_lowbias32({x}u));' for x in (0, 1, 2, 0x9e3779b9, 0xffffffff, 12345)]
    lines += ["  return wgs_add_particles == NULL || wgs_set_emitters == NULL;", "}"]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines) + "\n")
    # (compiled, not linked against the library: the addresses are taken in a translation unit of their own)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-Wno-address", f"-DWGS_DIM={dim}", f"-I{abi.INCLUDE}", "-c", str(src), "-o", str(tmp_path / "probe.o")], check=True)
    src.write_text("\n".join(lines).replace("return wgs_add_particles == NULL || wgs_set_emitters == NULL;", "return 0;") + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", f"-DWGS_DIM={dim}", f"-I{abi.INCLUDE}", str(src), "-o", str(exe)], check=True)
    out = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert ["S", str(SIZE[dim]), str(PARTICLE[dim])] in out and ["C", "8"] in out
    assert {l[1]: (int(l[2]), int(l[3])) for l in out if l[0] == "F"} == offsets(dim)
    assert [int(l[1]) for l in out if l[0] == "H"] == [ET.lowbias32_int(x) for x in (0, 1, 2, 0x9e3779b9, 0xffffffff, 12345)]


@pytest.mark.parametrize("dim", [2, 3])
def test_ctypes_twin_and_prototypes(dim):
    from wgsparkl_amd import _ffi, models
    T = _ffi.make_types(dim)
    ct = _ffi.emitter_type(T, dim)
    assert C.sizeof(ct) == SIZE[dim] and [f for f, _ in ct._fields_] == FIELDS
    assert {f: (getattr(ct, f).offset, getattr(ct, f).size) for f in FIELDS} == offsets(dim)
    protos = _ffi.emit_prototypes(T, dim)
    assert list(protos) == list(EXT.functions)
    for name, (ret, params) in EXT.functions.items():
        restype, argtypes = protos[name]
        assert (abi.ctypes_kind(restype), [abi.ctypes_kind(t) for t in argtypes]) == (abi.return_kind(ret), abi.param_kinds(params)), name
    assert not set(protos) & set(_ffi.prototypes(T)) and not set(protos) & set(_ffi.EXPORTS)
    assert _ffi.MAX_EMITTERS == models.MAX_EMITTERS == 8


@pytest.mark.parametrize("dim", [2, 3])
def test_the_loaded_library_carries_the_prototypes(hip_libs, dim):
    lib, T = hip_libs.load(dim)
    for name, (restype, argtypes) in hip_libs.emit_prototypes(T, dim).items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


@pytest.mark.parametrize("dim", [2, 3])
def test_rust_file_is_the_extension_headers(dim):
    text = abi.read(RUST_PATH)
    rust = abi.rust_layout(abi.read(abi.RUST_PATH) + "\n" + text, dim)      # (the emitter holds a wgs_particle: lib.rs's)
    assert rust.size["wgs_emitter"] == SIZE[dim] and rust.fields["wgs_emitter"] == offsets(dim)
    assert abi.rust_layout(text.replace("pub proto: wgs_particle,", ""), dim).const == {"WGS_MAX_EMITTERS": 8}
    fns = abi.rust_functions(text)
    assert list(fns) == list(EXT.functions)
    for name, (ret, params) in EXT.functions.items():
        assert fns[name] == (abi.return_kind(ret), abi.param_kinds(params)), name
    for line in ("x = x.wrapping_mul(0x7feb352d);", "x = x.wrapping_mul(0x846ca68b);", "x ^= x >> 15;"):
        assert line in text
    lib_rs = abi.read(abi.RUST_PATH)
    assert "pub mod emit;" in lib_rs and "wgs_emitter" not in lib_rs


def test_cpp_wrapper_wraps_them_all():
    hpp = abi.read(abi.HPP_PATH)
    for name in EXT.functions:
        assert name + "(" in hpp, name
    for said in ("static MpmData create_reserved(", "void add_particles(const std::vector<wgs_particle> &particles, const std::vector<uint8_t> &models = {})",
                 "void set_emitters(const std::vector<wgs_emitter> &emitters)", "std::vector<wgs_emitter> emitters()", "uint32_t particle_capacity()"):
        assert said in hpp, said


@pytest.mark.parametrize("dim", [2, 3])
def test_calls_without_a_handle_fail_through_the_status_path(hip_libs, dim):
    """No wgs_data can be created without a GPU: a NULL handle is WGS_ERR_INVALID_ARGUMENT with a message, and nothing is written."""
    lib, T = hip_libs.load(dim)
    E = hip_libs.emitter_type(T, dim)
    arr = (E * hip_libs.MAX_EMITTERS)()
    C.memset(arr, 0x5a, C.sizeof(arr))
    n, cap = C.c_uint32(0x5a5a5a5a), C.c_uint32(0x5a5a5a5a)
    counts = (C.c_uint64 * 8)(*([7] * 8))
    part = (T.Particle * 1)()
    for call in (lambda: lib.wgs_add_particles(None, part, None, 1), lambda: lib.wgs_set_emitters(None, arr, 1), lambda: lib.wgs_set_emitters(None, None, 0),
                 lambda: lib.wgs_get_emitters(None, arr, C.byref(n)), lambda: lib.wgs_get_emitter_counts(None, counts, counts),
                 lambda: lib.wgs_get_particle_capacity(None, C.byref(cap))):
        assert call() == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_last_error()
    assert bytes(arr) == b"\x5a" * C.sizeof(arr) and n.value == cap.value == 0x5a5a5a5a and list(counts) == [7] * 8
    # without a device, creation fails before anything is made: the handle stays NULL
    h = C.c_void_p(0x5a)
    assert lib.wgs_data_create_reserved(None, None, None, 0, None, 0, 1.0, 64, 128, C.byref(h)) == hip_libs.ERR_INVALID_ARGUMENT


def _proto(dim, vel=None):
    from wgsparkl_amd.models import ElasticCoefficients
    from wgsparkl_amd.solver import ParticleSet
    ps = ParticleSet.uniform(np.zeros((1, dim), np.float32), 0.25, 1000.0, ElasticCoefficients.from_young_modulus(1e5, 0.3))
    if vel is not None:
        ps.vel[0] = vel
    return ps


def test_emitter_validation_and_the_nozzle():
    from wgsparkl_amd.models import MODEL_FLUID, Emitter
    from wgsparkl_amd.pipeline import MpmData
    for m in ("add_particles", "set_emitters", "emitters", "emitter_counts"):
        assert callable(getattr(MpmData, m))
    assert isinstance(MpmData.particle_capacity, property) and isinstance(MpmData.n, property)
    e = Emitter(_proto(3), (0.0, 1.0, 2.0), (2, 3, 4), 0.5, model=MODEL_FLUID, jitter=0.5, seed=9, start_substep=3, period=2, batches=5)
    assert e.batch_size == 24 and e.model == MODEL_FLUID
    bad = [dict(period=0), dict(period=1.5), dict(jitter=-0.1), dict(jitter=0.6), dict(jitter=float("nan")), dict(count=(2, 0, 1)), dict(count=(2, 2)),
           dict(lo=(0.0, 1.0)), dict(model=3), dict(seed=-1), dict(batches=2 ** 32), dict(spacing=float("inf"))]
    for kw in bad:
        args = dict(lo=(0.0, 1.0, 2.0), count=(2, 3, 4), spacing=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            Emitter(_proto(3), **args)
    from wgsparkl_amd.solver import ParticleSet
    two = _proto(3)
    two = ParticleSet(**{k: (np.repeat(v, 2, axis=0) if isinstance(v, np.ndarray) else v) for k, v in two.__dict__.items()})
    with pytest.raises(ValueError):
        Emitter(two, (0.0, 1.0, 2.0), (2, 3, 4), 0.5)
    # period = ceil(thickness / (|v| dt)): one row of spacing 0.5 falling at 75 per second with dt = 1/1200 clears the nozzle in 8 substeps
    nz = Emitter.nozzle(_proto(3, vel=(0.0, -75.0, 0.0)), (0.0, 5.0, 0.0), (4, 1, 4), 0.5, 1.0 / 1200.0, jitter=0.1, batches=7)
    assert (nz.period, nz.batches, nz.jitter, nz.count) == (8, 7, 0.1, (4, 1, 4))
    assert Emitter.nozzle(_proto(2, vel=(3.0, -4.0)), (0.0, 0.0), (2, 6), 0.25, 0.01).period == 30           # 6 * 0.25 / (5 * 0.01)
    assert Emitter.nozzle(_proto(2, vel=(0.0, -4.0)), (0.0, 0.0), (2, 6), 0.25, 0.01, thickness=0.41).period == 11
    assert Emitter.nozzle(_proto(2, vel=(0.0, -400.0)), (0.0, 0.0), (2, 1), 0.25, 0.01).period == 1
    with pytest.raises(ValueError):
        Emitter.nozzle(_proto(2), (0.0, 0.0), (2, 1), 0.25, 0.01)                                            # no velocity: no period


def test_scene_keys_the_new_scenes_and_the_documents():
    from wgsparkl_amd import scenes
    from wgsparkl_amd.models import MODEL_FLUID
    from wgsparkl_amd.sharded import NativeShard
    doc = scenes.__doc__
    assert "| `particle_capacity` |" in doc and "| `emitters` |" in doc and doc.index("| `forces` |") < doc.index("| `particle_capacity` |") < doc.index("| `emitters` |")
    for dim in (2, 3):
        sc = scenes.faucet(dim, batches=5)
        em = sc["emitters"][0]
        assert sc["particles"].n == 0 and sc["particles"].dim == dim and sc["model"] == MODEL_FLUID and sc["colliders"] == []
        assert sc["particle_capacity"] == 5 * em.batch_size and em.batches == 5 and em.period == 8 and em.proto.vel[0, 1] < 0
        assert sum(w is not None for w in sc["walls"]) == 2 * dim - 1
        sp = scenes.sand_pour(dim, batches=4)
        em = sp["emitters"][0]
        ps = sp["particles"]
        assert ps.n > 0 and ps.has_plasticity.all() and len(sp["colliders"]) == 1 and sp["particle_capacity"] == ps.n + 4 * em.batch_size
        for f in ("mass", "init_volume", "lambda_", "mu", "dp", "phase"):          # bit for bit the heap's material
            assert np.array_equal(getattr(em.proto, f)[0], getattr(ps, f)[0]), f
        # a slab refuses both keys before it touches the library
        for key, other in (("particle_capacity", "emitters"), ("emitters", "particle_capacity")):
            slab_scene = {k: v for k, v in sp.items() if k != other}       # (sand_pour: no other single-domain key)
            with pytest.raises(ValueError, match=key):
                NativeShard.from_scene(None, slab_scene, 0)
    for make in (scenes.dam_break, scenes.block_in_fluid, scenes.walled_box, scenes.snowball, scenes.planetoid, scenes.vortex_tank,
                 scenes.reference_smoke_scene, lambda: scenes.neo_hookean_cube(n_side=4), lambda: scenes.sand_column(4, 4, 4)):
        assert "emitters" not in make() and "particle_capacity" not in make()
    for doc, said in (("INTEGRATION.md", "wgs_add_particles"), ("INTEGRATION.md", "wgs_set_emitters"), ("README.md", "wgs_add_particles"),
                      ("DESIGN.md", "## 7f. Particles added at run time"), ("DESIGN.md", "k_append"), ("tools/README.md", "gpu_emit_prof.py"),
                      ("notes/round_34.md", "kernel_symbols_cmp")):
        assert said in abi.read(os.path.join(abi.ROOT, doc)), (doc, said)
