"""ctypes binding of the C ABI (include/wgsparkl_hip.h) — one CDLL per dimension.

The library is the product; this module is the thinnest possible host glue.
It fails loudly when the HIP extension is missing: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")

WGS_OK = 0
# wgs_status (include/wgsparkl_hip.h WGS_ERR_*): what WgsError.code and a raw call's return value compare with
ERR_INVALID_ARGUMENT, ERR_NO_DEVICE, ERR_HIP, ERR_GRID_OVERFLOW, ERR_KEY_RANGE, ERR_UNSUPPORTED = 1, 2, 3, 4, 5, 6
ABI_VERSION = 7  # include/wgsparkl_hip.h WGS_ABI_VERSION
WGS_NUM_PASSES = 10
PASS_NAMES = ("update rigid particles", "grid sort", "grid_update_cdf", "p2g_cdf", "g2p_cdf", "p2g",
              "grid_update", "g2p", "particles_update", "integrate_bodies")  # src/pipeline.rs:201-271


class WgsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"wgsparkl_hip error {code}: {msg}")
        self.code = code


# Developer override, read once per process like WGS_DEBUG and WGS_REHASH_PERIOD: a directory that holds both libraries of
# a variant (tools/build_variant.sh). A variant is chosen by path, never by copying it over the tree's libraries.
_LIB_DIR = os.environ.get("WGS_LIB_DIR") or None


def lib_path(dim: int) -> str:
    return os.path.join(_LIB_DIR or _CSRC, f"libwgsparkl{dim}d_hip.so")


def build(force: bool = False) -> None:
    """hipcc --offload-arch=gfx950 build of both libraries (csrc/build.sh)."""
    cmd = ["bash", os.path.join(_CSRC, "build.sh")] + (["force"] if force else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building the HIP extension failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])


def make_types(D: int):
    f = C.c_float
    u = C.c_uint32

    class SimParams(C.Structure):
        _fields_ = [("gravity", f * D), ("dt", f)]

    class Elastic(C.Structure):
        _fields_ = [("lambda_", f), ("mu", f)]

    class DruckerPrager(C.Structure):
        _fields_ = [("h0", f), ("h1", f), ("h2", f), ("h3", f), ("lambda_", f), ("mu", f)]

    class PlasticState(C.Structure):
        _fields_ = [("plastic_deformation_gradient_det", f), ("plastic_hardening", f), ("log_vol_gain", f)]

    class Phase(C.Structure):
        _fields_ = [("phase", f), ("max_stretch", f)]

    class Cdf(C.Structure):
        _fields_ = [("normal", f * D), ("rigid_vel", f * D), ("signed_distance", f), ("affinity", u)]

    class Dynamics(C.Structure):
        _fields_ = [("velocity", f * D), ("def_grad", f * (D * D)), ("affine", f * (D * D)), ("cdf", Cdf),
                    ("init_volume", f), ("init_radius", f), ("mass", f)]

    class Particle(C.Structure):
        _fields_ = [("position", f * D), ("dynamics", Dynamics), ("model", Elastic), ("has_plasticity", u),
                    ("plasticity", DruckerPrager), ("has_phase", u), ("phase", Phase)]

    class Pose(C.Structure):
        _fields_ = [("rotation", f * 4), ("translation", f * 3), ("scale", f)]

    class Velocity(C.Structure):
        _fields_ = [("linear", f * 3), ("angular", f * 3)]

    class Collider(C.Structure):
        _fields_ = [("shape_type", u), ("shape", f * 4), ("pose", Pose), ("velocity", Velocity), ("com", f * 3)]

    class MassProperties(C.Structure):
        _fields_ = [("inv_mass", f * 3), ("inv_inertia_local", f * 9)]

    class NodeRecord(C.Structure):
        _fields_ = [("cell", C.c_int32 * D), ("velocity", f * D), ("mass", f), ("cdf_distance", f),
                    ("cdf_affinities", u), ("cdf_closest_id", u)]

    class BlockRecord(C.Structure):
        _fields_ = [("virtual_id", C.c_int32 * D), ("first_particle", u), ("num_particles", u)]

    class Stats(C.Structure):
        _fields_ = [("num_particles", u), ("num_active_blocks", u), ("grid_capacity", u), ("overflow", u),
                    ("substeps_done", C.c_uint64), ("device_bytes", C.c_uint64), ("num_near_collider_blocks", u), ("grid_growths", u),
                    ("cell_changers", C.c_uint64), ("table_rebuilds", C.c_uint64),
                    ("block_ids", u), ("block_ids_free", u), ("table_marks", u), ("table_refreshes", u)]

    class GridSample(C.Structure):
        _fields_ = [("velocity", f * D), ("velocity_gradient", f * (D * D)), ("density", f), ("active_nodes", u)]

    class ParticleField(C.Structure):
        _fields_ = [("stress", f * (D * D)), ("mean_stress", f), ("von_mises", f), ("volume_ratio", f), ("stretch", f * D), ("model", u)]

    ns = dict(SimParams=SimParams, Elastic=Elastic, DruckerPrager=DruckerPrager, PlasticState=PlasticState,
              Phase=Phase, Cdf=Cdf, Dynamics=Dynamics, Particle=Particle, Pose=Pose, Velocity=Velocity,
              Collider=Collider, MassProperties=MassProperties, NodeRecord=NodeRecord, BlockRecord=BlockRecord, Stats=Stats,
              GridSample=GridSample, ParticleField=ParticleField)
    return type("Types", (), ns)


class DevicePtrs(C.Structure):
    """wgs_device_ptrs (include/wgsparkl_hip.h): the optional interop view of the particle state on the device."""
    _fields_ = [("position_quads", C.c_void_p), ("particle_ids", C.c_void_p), ("count", C.c_uint32), ("capacity", C.c_uint32),
                ("dim", C.c_uint32), ("reserved", C.c_uint32), ("hip_stream", C.c_void_p)]


class Wall(C.Structure):
    """wgs_wall (include/wgsparkl_hip.h "Domain walls"): one face; the same struct in both dimensions."""
    _fields_ = [("type", C.c_uint32), ("friction", C.c_float), ("plane", C.c_int32)]


WALL_NONE, WALL_STICKY, WALL_SLIP, WALL_SEPARATE = 0, 1, 2, 3   # WGS_WALL_*


# wgs_diagnostics (include/wgsparkl_hip.h "Device-side diagnostics"): the same struct in both dimensions
DIAG_PARTICLES, DIAG_ENERGY, DIAG_GRID, DIAG_DIGEST = 1, 2, 4, 8
DIAG_ALL = DIAG_PARTICLES | DIAG_ENERGY | DIAG_GRID | DIAG_DIGEST
SUM_INDEX = dict(mass=0, momentum=1, angular=4, mass_moment=7, kinetic=10, kinetic_affine=11, elastic=12, gravity_potential=13,
                 grid_mass=14, grid_momentum=15, grid_angular=18)   # WGS_SUM_*
NUM_SUMS = 21


class FixedSum(C.Structure):
    """wgs_fixed_sum: value == ldexp(fixed, exponent)."""
    _fields_ = [("fixed", C.c_int64), ("exponent", C.c_int32), ("reserved", C.c_uint32), ("value", C.c_double)]


class Diagnostics(C.Structure):
    _fields_ = [("num_particles", C.c_uint64), ("num_nonfinite", C.c_uint64), ("sum", FixedSum * NUM_SUMS),
                ("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("max_speed", C.c_float), ("max_affine_norm", C.c_float),
                ("min_det_f", C.c_float), ("max_det_f", C.c_float), ("max_wave_speed", C.c_float), ("cfl", C.c_float),
                ("digest", C.c_uint64 * 2), ("what", C.c_uint32), ("model", C.c_uint32)]


def prototypes(T):
    """name -> (restype, argtypes) of every entry point of include/wgsparkl_hip.h, in the header's order; `T` = make_types(dim).
    `[]` is `(void)`; `st` is wgs_status. Handles (wgs_pipeline / wgs_data / wgs_comm *) and untyped buffers are void pointers."""
    P, vp, st, i32, u32, f32, size = C.POINTER, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_float, C.c_size_t
    fp, u8p, u32p = P(f32), P(C.c_uint8), P(u32)
    return {
        "wgs_last_error": (C.c_char_p, []),
        "wgs_dim": (i32, []),
        "wgs_build_info": (C.c_char_p, []),
        "wgs_abi_version": (u32, []),
        "wgs_pipeline_create": (st, [i32, P(vp)]),
        "wgs_pipeline_destroy": (None, [vp]),
        "wgs_data_create": (st, [vp, P(T.SimParams), P(T.Particle), size, P(T.Collider), size, f32, u32, P(vp)]),
        "wgs_data_destroy": (None, [vp]),
        "wgs_set_constitutive_model": (st, [vp, i32]),
        "wgs_set_fluid_eos": (st, [vp, f32]),
        "wgs_set_particle_models": (st, [vp, u8p]),
        "wgs_read_particle_models": (st, [vp, u8p]),
        "wgs_step": (st, [vp, vp, u32, i32]),
        "wgs_sync": (st, [vp]),
        "wgs_set_sim_params": (st, [vp, P(T.SimParams)]),
        "wgs_set_collider_poses": (st, [vp, P(T.Pose), fp, size]),
        "wgs_set_body_velocities": (st, [vp, P(T.Velocity), size]),
        "wgs_set_body_mass_properties": (st, [vp, P(T.MassProperties), size]),
        "wgs_set_rigid_particles": (st, [vp, fp, vp, size, fp, u32p, size]),
        "wgs_read_body_poses": (st, [vp, P(T.Pose), P(T.Velocity), fp, size]),
        "wgs_read_positions": (st, [vp, fp]),
        "wgs_get_device_ptrs": (st, [vp, P(DevicePtrs)]),
        "wgs_read_particles": (st, [vp, P(T.Particle), P(T.PlasticState)]),
        "wgs_prep_vertex_buffer": (st, [vp, u32, vp]),
        "wgs_prep_vertex_buffer_device": (st, [vp, u32, vp]),
        "wgs_set_plastic_state": (st, [vp, P(T.PlasticState)]),
        "wgs_read_grid": (st, [vp, P(T.NodeRecord), size, P(size)]),
        "wgs_read_blocks": (st, [vp, P(T.BlockRecord), size, P(size), u32p]),
        "wgs_read_timings": (st, [vp, fp]),
        "wgs_read_timing_overhead": (st, [vp, fp]),
        "wgs_get_stats": (st, [vp, P(T.Stats)]),
        "wgs_set_uniform_material": (st, [vp, f32, f32, f32, f32]),
        "wgs_set_grid_growth": (st, [vp, i32]),
        "wgs_set_domain_walls": (st, [vp, P(Wall)]),
        "wgs_get_domain_walls": (st, [vp, P(Wall)]),
        # the plasticity rule of the data (Drucker-Prager | snow; no reference counterpart)
        "wgs_set_plasticity_model": (st, [vp, i32]),
        "wgs_get_plasticity_model": (st, [vp, P(i32)]),
        "wgs_debug_scan": (st, [vp, u32p, u32, u32p, u32p]),
        # multi-GPU (x-slab decomposition; new design, no reference counterpart)
        "wgs_data_create_sharded": (st, [vp, P(T.SimParams), P(T.Particle), size, u32p, P(T.Collider), size, f32, u32, u32,
                                         i32, i32, i32, P(vp)]),
        "wgs_shard_halo_record_bytes": (u32, []),
        "wgs_shard_particle_record_bytes": (u32, []),
        "wgs_shard_buffer_header_bytes": (u32, []),
        "wgs_set_stream": (st, [vp, vp]),
        "wgs_shard_export": (st, [vp, vp, u32, u32p]),
        "wgs_comm_get_unique_id": (st, [C.c_char_p]),
        "wgs_comm_create": (st, [vp, C.c_char_p, i32, i32, i32, P(vp)]),
        "wgs_comm_destroy": (None, [vp]),
        "wgs_shard_attach": (st, [vp, vp, i32, i32, u32, u32]),
        "wgs_sharded_step": (st, [vp, vp, u32]),
        "wgs_sharded_step_lockstep": (st, [vp, P(vp), u32, u32]),
        # device-side diagnostics (reproducible sums, bounds, state digest; no reference counterpart)
        "wgs_read_diagnostics": (st, [vp, u32, P(Diagnostics)]),
        "wgs_enqueue_diagnostics": (st, [vp, u32, vp]),
        # Lagrangian field output (per-particle stress and strain of the stored state; no reference counterpart)
        "wgs_read_particle_fields": (st, [vp, P(T.ParticleField)]),
        "wgs_read_particle_fields_device": (st, [vp, vp]),
        # Eulerian field output (the grid sampled at points, a dense window of its nodes; no reference counterpart)
        "wgs_sample_grid": (st, [vp, fp, size, P(T.GridSample)]),
        "wgs_sample_grid_device": (st, [vp, vp, size, vp]),
        "wgs_read_grid_window": (st, [vp, P(i32), u32p, fp]),
        "wgs_read_grid_window_device": (st, [vp, P(i32), u32p, vp]),
    }


EXPORTS = tuple(prototypes(make_types(3)))   # the names do not depend on the dimension


class ForceField(C.Structure):
    """wgs_force_field (include/wgsparkl_hip_forces.h): one force field; the same 68 bytes in both dimensions."""
    _fields_ = [("kind", C.c_uint32), ("falloff", C.c_uint32), ("region", C.c_uint32), ("strength", C.c_float), ("softening", C.c_float),
                ("center", C.c_float * 3), ("vec", C.c_float * 3), ("region_center", C.c_float * 3), ("region_half", C.c_float * 3)]


FORCE_NONE, FORCE_UNIFORM, FORCE_RADIAL, FORCE_VORTEX, FORCE_DRAG = 0, 1, 2, 3, 4   # WGS_FORCE_*
REGION_ALL, REGION_BOX, REGION_BALL = 0, 1, 2                                        # WGS_REGION_*
MAX_FORCE_FIELDS = 8                                                                 # WGS_MAX_FORCE_FIELDS


def forces_prototypes():
    """name -> (restype, argtypes) of the entry points of the extension header include/wgsparkl_hip_forces.h, in its order (apart from
    prototypes(): that table is the main header's, entry for entry)."""
    vp, st, u32 = C.c_void_p, C.c_int32, C.c_uint32
    return {
        "wgs_set_force_fields": (st, [vp, C.POINTER(ForceField), u32]),
        "wgs_get_force_fields": (st, [vp, C.POINTER(ForceField), C.POINTER(u32)]),
    }


MAX_EMITTERS = 8   # WGS_MAX_EMITTERS


def lowbias32(x):
    """wgs_lowbias32 (include/wgsparkl_hip_emit.h), on numpy uint32 arrays or Python ints."""
    import numpy as np
    x = np.asarray(x, np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def emitter_type(T, D: int):
    """wgs_emitter (include/wgsparkl_hip_emit.h) over the particle struct of `T` = make_types(D): 240 bytes in 3D, 176 in 2D."""
    if not hasattr(T, "Emitter"):
        class Emitter(C.Structure):
            _fields_ = [("proto", T.Particle), ("model", C.c_uint8), ("lo", C.c_float * D), ("count", C.c_uint32 * D), ("spacing", C.c_float),
                        ("jitter", C.c_float), ("seed", C.c_uint32), ("start_substep", C.c_uint32), ("period", C.c_uint32), ("batches", C.c_uint32)]
        T.Emitter = Emitter
    return T.Emitter


def emit_prototypes(T, D: int):
    """name -> (restype, argtypes) of the entry points of the extension header include/wgsparkl_hip_emit.h, in its order (apart from
    prototypes(), like forces_prototypes())."""
    P, vp, st, u32, f32, size = C.POINTER, C.c_void_p, C.c_int32, C.c_uint32, C.c_float, C.c_size_t
    E = emitter_type(T, D)
    return {
        "wgs_data_create_reserved": (st, [vp, P(T.SimParams), P(T.Particle), size, P(T.Collider), size, f32, u32, u32, P(vp)]),
        "wgs_get_particle_capacity": (st, [vp, P(u32)]),
        "wgs_add_particles": (st, [vp, P(T.Particle), P(C.c_uint8), size]),
        "wgs_set_emitters": (st, [vp, P(E), u32]),
        "wgs_get_emitters": (st, [vp, P(E), P(u32)]),
        "wgs_get_emitter_counts": (st, [vp, P(C.c_uint64), P(C.c_uint64)]),
    }


class Sink(C.Structure):
    """wgs_sink (include/wgsparkl_hip_remove.h): a region, a side and a schedule; the same 40 bytes in both dimensions."""
    _fields_ = [("region", C.c_uint32), ("side", C.c_uint32), ("center", C.c_float * 3), ("half", C.c_float * 3),
                ("start_substep", C.c_uint32), ("period", C.c_uint32)]


MAX_SINKS = 8                        # WGS_MAX_SINKS
SINK_INSIDE, SINK_OUTSIDE = 0, 1     # WGS_SINK_*


def remove_prototypes():
    """name -> (restype, argtypes) of the entry points of the extension header include/wgsparkl_hip_remove.h, in its order (apart from
    prototypes(), like forces_prototypes())."""
    P, vp, st, u32, u8p = C.POINTER, C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint8)
    return {
        "wgs_remove_particles": (st, [vp, u8p, P(u32), P(u32)]),
        "wgs_remove_particles_device": (st, [vp, vp, vp, P(u32)]),
        "wgs_remove_particles_in": (st, [vp, P(Sink), u32, P(u32), P(u32)]),
        "wgs_set_sinks": (st, [vp, P(Sink), u32]),
        "wgs_get_sinks": (st, [vp, P(Sink), P(u32)]),
        "wgs_get_sink_counts": (st, [vp, P(C.c_uint64)]),
        "wgs_debug_compact_map": (st, [vp, u8p, u32, P(u32), P(u32)]),
    }


_LIBS = {}


def load(dim: int):
    """Load libwgsparkl{dim}d_hip.so; raises if it has not been built."""
    if dim in _LIBS:
        return _LIBS[dim]
    path = lib_path(dim)
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing — run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc, gfx950). There is no CPU fallback for the MPM step.")
    # PyTorch-ROCm ships its own libamdhip64; if this library pulled in /opt/rocm's copy first, a later
    # torch.cuda init would find a second HIP runtime and report "No HIP GPUs are available". Loading torch
    # first makes both resolve to one runtime (torch is only plumbing here: streams, torch.distributed).
    try:
        import torch  # noqa: F401
    except Exception:  # torch is optional for the single-GPU path
        pass
    if _LIB_DIR:   # nothing produced from a variant is silent about it
        print(f"wgsparkl_amd: WGS_LIB_DIR in force, loading {os.path.basename(path)} from {_LIB_DIR}", file=sys.stderr, flush=True)
    lib = C.CDLL(path)
    T = make_types(dim)
    for name, (restype, argtypes) in {**prototypes(T), **forces_prototypes(), **emit_prototypes(T, dim), **remove_prototypes()}.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if lib.wgs_abi_version() != ABI_VERSION:   # (the structs carry no size field: include/wgsparkl_hip.h WGS_ABI_VERSION)
        raise RuntimeError(f"{path}: ABI version {lib.wgs_abi_version()}, this binding mirrors {ABI_VERSION} — rebuild the library (csrc/build.sh)")
    assert lib.wgs_dim() == dim
    _LIBS[dim] = (lib, T)
    return _LIBS[dim]


def check(lib, status):
    if status != WGS_OK:
        msg = lib.wgs_last_error()
        raise WgsError(status, msg.decode() if msg else "")
