"""`MpmPipeline` / `MpmData` — host-side mirror of `wgsparkl::pipeline`
(reference: src/pipeline.rs:24-281) over the C ABI of include/wgsparkl_hip.h.

The reference records ~25 dispatches into a `KernelInvocationQueue` once
(`queue_step`) and the caller replays that queue `num_substeps` times per frame
(src_testbed/step.rs:122-128). The same call shape is kept here:

    pipeline = MpmPipeline(device=0, dim=3)
    data = MpmData.new(pipeline, params, particles, colliders, cell_width, grid_capacity)
    queue = KernelInvocationQueue()
    pipeline.queue_step(data, queue, add_timestamps=False)
    for _ in range(num_substeps):
        queue.encode()          # enqueue one substep on the data's HIP stream
    data.sync()                 # device.poll(Maintain::Wait)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np

from . import _ffi
from .models import MODEL_COROTATED
from .solver import Collider, ParticleSet, SimulationParams

F32 = np.float32


@dataclass
class FixedSum:
    """One reproducible sum: `value == ldexp(fixed, exponent)`; `fixed` sums of equal exponent add exactly (ranks of a sharded run)."""
    fixed: np.ndarray       # int64, one entry per component
    exponent: int
    value: np.ndarray       # float64

    def __float__(self):
        return float(self.value[0])


@dataclass
class Diagnostics:
    """`wgs_diagnostics` as numpy: what the simulation says about itself without a read-back (include/wgsparkl_hip.h "Device-side
    diagnostics"). `sums[name]` for name in _ffi.SUM_INDEX; vector sums have `dim` components (angular: 1 in 2D)."""
    dim: int
    num_particles: int
    num_nonfinite: int
    sums: Dict[str, FixedSum]
    aabb_min: np.ndarray
    aabb_max: np.ndarray
    max_speed: float
    max_affine_norm: float
    min_det_f: float
    max_det_f: float
    max_wave_speed: float
    cfl: float
    digest: tuple
    what: int
    model: int
    raw: bytes              # the struct itself: two runs ended in the same state iff these bytes are equal

    def value(self, name: str) -> np.ndarray:
        return self.sums[name].value

    def suggest_dt(self, dt: float, cfl_target: float = 0.5, cell_width: Optional[float] = None) -> float:
        """The time step that would put the fastest signal of the current state at `cfl_target` cells per step: material velocity
        (`cfl` was measured with the `dt` passed here) and, when `cell_width` is given, the elastic wave on top of it. Arithmetic on
        the result only; `dt` is returned unchanged when nothing moves."""
        per_dt = self.cfl / dt if dt > 0 else 0.0                    # max |v|_inf / h
        if cell_width:
            per_dt += self.max_wave_speed / float(cell_width)
        return float(cfl_target / per_dt) if per_dt > 0 else float(dt)


@dataclass
class GridSamples:
    """`wgs_grid_sample` records as numpy (include/wgsparkl_hip.h "Eulerian field output"), one row per point."""
    velocity: np.ndarray            # [n, D]
    velocity_gradient: np.ndarray   # [n, D, D] (row, col)
    density: np.ndarray             # [n]
    active_nodes: np.ndarray        # [n] uint32: stencil nodes that lie in an active block
    raw: np.ndarray                 # [n, D + D*D + 2] uint32: the records themselves


def grid_samples_from_words(words: np.ndarray, dim: int) -> GridSamples:
    """`words`: [n, D + D*D + 2] uint32, the records as the library wrote them (the gradient is column-major there)."""
    D = dim
    fl = words.view(F32)
    return GridSamples(velocity=fl[:, :D].copy(), velocity_gradient=fl[:, D:D + D * D].reshape(-1, D, D).transpose(0, 2, 1).copy(),
                       density=fl[:, D + D * D].copy(), active_nodes=words[:, D + D * D + 1].copy(), raw=words)


@dataclass
class ParticleFields:
    """`wgs_particle_field` records as numpy (include/wgsparkl_hip.h "Lagrangian field output"), one row per particle in the
    caller's order."""
    stress: np.ndarray         # [n, D, D] (row, col): Kirchhoff stress of the stored state
    mean_stress: np.ndarray    # [n]: tr(stress) / D
    von_mises: np.ndarray      # [n]: sqrt(3/2) |dev stress|_F
    volume_ratio: np.ndarray   # [n]: J
    stretch: np.ndarray        # [n, D]: signed singular values of def_grad (fluid: cbrt / sqrt of J)
    model: np.ndarray          # [n] uint32: the model the stress was evaluated under
    raw: np.ndarray            # [n, D*D + D + 4] uint32: the records themselves


def particle_fields_from_words(words: np.ndarray, dim: int) -> ParticleFields:
    """`words`: [n, D*D + D + 4] uint32, the records as the library wrote them (the stress is column-major there)."""
    D, DD = dim, dim * dim
    fl = words.view(F32)
    return ParticleFields(stress=fl[:, :DD].reshape(-1, D, D).transpose(0, 2, 1).copy(), mean_stress=fl[:, DD].copy(),
                          von_mises=fl[:, DD + 1].copy(), volume_ratio=fl[:, DD + 2].copy(), stretch=fl[:, DD + 3:DD + 3 + D].copy(),
                          model=words[:, DD + 3 + D].copy(), raw=words)


def diagnostics_from_struct(r, dim: int) -> Diagnostics:
    ncomp = dict(momentum=dim, mass_moment=dim, grid_momentum=dim, angular=1 if dim == 2 else 3, grid_angular=1 if dim == 2 else 3)
    sums = {}
    for name, i in _ffi.SUM_INDEX.items():
        k = ncomp.get(name, 1)
        sums[name] = FixedSum(np.array([r.sum[i + c].fixed for c in range(k)], np.int64), int(r.sum[i].exponent),
                              np.array([r.sum[i + c].value for c in range(k)], np.float64))
    return Diagnostics(dim=dim, num_particles=int(r.num_particles), num_nonfinite=int(r.num_nonfinite), sums=sums,
                       aabb_min=np.array(list(r.aabb_min)[:dim], F32), aabb_max=np.array(list(r.aabb_max)[:dim], F32),
                       max_speed=float(r.max_speed), max_affine_norm=float(r.max_affine_norm), min_det_f=float(r.min_det_f),
                       max_det_f=float(r.max_det_f), max_wave_speed=float(r.max_wave_speed), cfl=float(r.cfl),
                       digest=(int(r.digest[0]), int(r.digest[1])), what=int(r.what), model=int(r.model), raw=bytes(r))


def read_diagnostics(lib, handle, dim: int, what: int) -> Diagnostics:
    r = _ffi.Diagnostics()
    _ffi.check(lib, lib.wgs_read_diagnostics(handle, int(what), C.byref(r)))
    return diagnostics_from_struct(r, dim)


class KernelInvocationQueue:
    """Stand-in for wgcore's KernelInvocationQueue: holds the recorded step so it can
    be replayed with `encode()` (src_testbed/step.rs:126-128)."""

    def __init__(self):
        self._recorded = []

    def _push(self, fn):
        self._recorded.append(fn)

    def clear(self):
        self._recorded.clear()

    def encode(self, num_replays: int = 1):
        for fn in self._recorded:
            fn(num_replays)


class MpmPipeline:
    """src/pipeline.rs:24-39,176-193. `MpmPipeline.new(device)` fails when the HIP
    extension or a HIP device is missing (reference: ComposerError)."""

    def __init__(self, device: int = 0, dim: int = 3):
        self.dim = dim
        self.lib, self.T = _ffi.load(dim)
        h = C.c_void_p()
        _ffi.check(self.lib, self.lib.wgs_pipeline_create(int(device), C.byref(h)))
        self._h = h
        self.device = device

    new = classmethod(lambda cls, device=0, dim=3: cls(device, dim))

    def queue_step(self, data: "MpmData", queue: KernelInvocationQueue, add_timestamps: bool = False):
        """src/pipeline.rs:195-281 — records one substep; nothing runs until `queue.encode()`."""
        def run(n):
            _ffi.check(self.lib, self.lib.wgs_step(self._h, data._h, int(n), 1 if add_timestamps else 0))
        queue._push(run)

    def step(self, data: "MpmData", num_substeps: int = 1, timestamps: bool = False):
        """queue_step + encode x num_substeps in one call."""
        _ffi.check(self.lib, self.lib.wgs_step(self._h, data._h, int(num_substeps), 1 if timestamps else 0))

    def close(self):
        if getattr(self, "_h", None):
            self.lib.wgs_pipeline_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pack_particles(T, ps: ParticleSet):
    """ParticleSet -> contiguous array of wgs_particle (the repr(C) image of `Particle`)."""
    n, D = ps.n, ps.dim
    words = C.sizeof(T.Particle) // 4
    raw = np.zeros((n, words), np.float32)
    u = raw.view(np.uint32)
    off = lambda path: _offset_words(T.Particle, path)
    raw[:, off("position"):off("position") + D] = ps.pos
    o = off("dynamics.velocity"); raw[:, o:o + D] = ps.vel
    o = off("dynamics.def_grad"); raw[:, o:o + D * D] = ps.def_grad
    o = off("dynamics.affine"); raw[:, o:o + D * D] = ps.affine
    o = off("dynamics.cdf.normal"); raw[:, o:o + D] = ps.cdf_normal
    o = off("dynamics.cdf.rigid_vel"); raw[:, o:o + D] = ps.cdf_rigid_vel
    raw[:, off("dynamics.cdf.signed_distance")] = ps.cdf_dist
    u[:, off("dynamics.cdf.affinity")] = ps.cdf_affinity
    raw[:, off("dynamics.init_volume")] = ps.init_volume
    raw[:, off("dynamics.init_radius")] = ps.init_radius
    raw[:, off("dynamics.mass")] = ps.mass
    raw[:, off("model.lambda_")] = ps.lambda_
    raw[:, off("model.mu")] = ps.mu
    hp = ps.has_plasticity if ps.has_plasticity is not None else np.ones(n, bool)
    hph = ps.has_phase if ps.has_phase is not None else np.ones(n, bool)
    u[:, off("has_plasticity")] = hp.astype(np.uint32)
    o = off("plasticity"); raw[:, o:o + 6] = ps.dp
    u[:, off("has_phase")] = hph.astype(np.uint32)
    o = off("phase"); raw[:, o:o + 2] = ps.phase
    return raw


def _offset_words(struct, path: str) -> int:
    off = 0
    cur = struct
    for name in path.split("."):
        fld = getattr(cur, name)
        off += fld.offset
        cur = dict((f[0], f[1]) for f in cur._fields_)[name]
    return off // 4


def _unpack_particles(T, raw: np.ndarray, D: int, plastic: Optional[np.ndarray]) -> ParticleSet:
    u = raw.view(np.uint32)
    off = lambda path: _offset_words(T.Particle, path)
    sl = lambda path, k: raw[:, off(path):off(path) + k].copy()
    n = raw.shape[0]
    return ParticleSet(
        dim=D, pos=sl("position", D), vel=sl("dynamics.velocity", D), def_grad=sl("dynamics.def_grad", D * D),
        affine=sl("dynamics.affine", D * D), cdf_normal=sl("dynamics.cdf.normal", D),
        cdf_rigid_vel=sl("dynamics.cdf.rigid_vel", D), cdf_dist=raw[:, off("dynamics.cdf.signed_distance")].copy(),
        cdf_affinity=u[:, off("dynamics.cdf.affinity")].copy(), init_volume=raw[:, off("dynamics.init_volume")].copy(),
        init_radius=raw[:, off("dynamics.init_radius")].copy(), mass=raw[:, off("dynamics.mass")].copy(),
        lambda_=raw[:, off("model.lambda_")].copy(), mu=raw[:, off("model.mu")].copy(), dp=sl("plasticity", 6),
        dp_state=plastic if plastic is not None else np.tile(np.array([1, 1, 0], F32), (n, 1)),
        phase=sl("phase", 2), has_plasticity=u[:, off("has_plasticity")] != 0, has_phase=u[:, off("has_phase")] != 0)


def _is_dynamic(c: Collider) -> bool:
    return any(float(v) != 0.0 for v in list(c.inv_mass) + list(c.inv_inertia_local))


def _fill_collider(T, dst, c: Collider, D: int):
    dst.shape_type = int(c.shape_type)
    sh = list(c.shape) + [0.0] * (4 - len(c.shape))
    dst.shape = (C.c_float * 4)(*sh)
    if D == 2:
        ang = F32(c.rotation[0])
        dst.pose.rotation = (C.c_float * 4)(float(np.cos(ang)), float(np.sin(ang)), 0.0, 0.0)
    else:
        dst.pose.rotation = (C.c_float * 4)(*c.rotation)
    t = list(c.translation) + [0.0] * (3 - len(c.translation))
    dst.pose.translation = (C.c_float * 3)(*t)
    dst.pose.scale = c.scale
    dst.velocity.linear = (C.c_float * 3)(*(list(c.linvel)[:D] + [0.0] * (3 - D)))
    dst.velocity.angular = (C.c_float * 3)(*((list(c.angvel) + [0.0, 0.0, 0.0])[:3]))
    com = list(c.com) if c.com is not None else list(c.translation)
    dst.com = (C.c_float * 3)(*(com + [0.0] * (3 - len(com))))


class DataHandle:
    """What is true of any `wgs_data *`, single-domain (`MpmData`) or one slab of a decomposition (`sharded.NativeShard`): the
    setters, the body and diagnostics read-backs and the handle's lifetime. A subclass's constructor creates the data and stores
    the handle in `self._h`."""

    def __init__(self, pipeline: MpmPipeline, colliders: Sequence[Collider]):
        self.pipeline, self.lib, self.T, self.dim = pipeline, pipeline.lib, pipeline.T, pipeline.dim
        self.n_colliders = len(colliders)
        self._h = None

    def _sim_params(self, params: SimulationParams):
        sp = self.T.SimParams()
        sp.gravity = (C.c_float * self.dim)(*params.gravity)
        sp.dt = params.dt
        return sp

    def _collider_array(self, colliders: Sequence[Collider]):
        cols = (self.T.Collider * max(1, len(colliders)))()
        for i, c in enumerate(colliders):
            _fill_collider(self.T, cols[i], c, self.dim)
        return cols

    # -- host -> device writes the caller performs every frame (src_testbed/step.rs:79-119, ui.rs:91-104)
    def set_constitutive_model(self, model: int):
        _ffi.check(self.lib, self.lib.wgs_set_constitutive_model(self._h, int(model)))

    def set_fluid_eos(self, gamma: float):
        """`wgs_set_fluid_eos`: the Tait exponent of MODEL_FLUID (default 7; finite and > 1). Stream-ordered; every rank
        of a sharded run passes the same value."""
        _ffi.check(self.lib, self.lib.wgs_set_fluid_eos(self._h, float(gamma)))

    def set_sim_params(self, params: SimulationParams):
        _ffi.check(self.lib, self.lib.wgs_set_sim_params(self._h, C.byref(self._sim_params(params))))

    def set_colliders(self, colliders: Sequence[Collider]):
        """Refresh poses + velocities of the coupled colliders."""
        n = len(colliders)
        tmp = self._collider_array(colliders)
        poses = (self.T.Pose * max(1, n))()
        vels = (self.T.Velocity * max(1, n))()
        coms = (C.c_float * (3 * max(1, n)))()
        for i in range(n):
            poses[i] = tmp[i].pose
            vels[i] = tmp[i].velocity
            for k in range(3):
                coms[3 * i + k] = tmp[i].com[k]
        _ffi.check(self.lib, self.lib.wgs_set_collider_poses(self._h, poses, coms, n))
        _ffi.check(self.lib, self.lib.wgs_set_body_velocities(self._h, vels, n))
        self.set_body_mass_properties(colliders)

    def set_rigid_particles(self, rb: dict):
        """`rb` = sampling.build_rigid_particles(...): local sample points, (vertex ids, collider) per sample, local
        mesh vertices and their collider (GpuRigidParticles + the shape vertex buffers)."""
        pts = np.ascontiguousarray(rb["local_pts"], F32)
        ids = np.ascontiguousarray(rb["ids"], np.uint32)
        vtx = np.ascontiguousarray(rb["local_vtx"], F32)
        vcol = np.ascontiguousarray(rb["vtx_collider"], np.uint32)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        _ffi.check(self.lib, self.lib.wgs_set_rigid_particles(
            self._h, pts.ctypes.data_as(fp), ids.ctypes.data_as(C.c_void_p), len(pts), vtx.ctypes.data_as(fp),
            vcol.ctypes.data_as(up), len(vtx)))

    def _set_mesh_samples(self, colliders: Sequence[Collider], cell_width: float):
        """Mesh colliders are sampled on the host like GpuRigidParticles::from_rapier (sampling step = cell width)."""
        from .sampling import build_rigid_particles
        rb = build_rigid_particles(colliders, self.dim, float(cell_width))
        if rb is not None:
            self.set_rigid_particles(rb)

    def set_body_mass_properties(self, colliders: Sequence[Collider]):
        """GpuBodySet::from_rapier's local mass properties: all zero = kinematic, else two-way coupling."""
        n = len(colliders)
        mp = (self.T.MassProperties * max(1, n))()
        for i, c in enumerate(colliders):
            im = (list(c.inv_mass) + [0.0] * 3)[:3]
            ii = (list(c.inv_inertia_local) + [0.0] * 9)[:9]
            mp[i].inv_mass = (C.c_float * 3)(*im)
            mp[i].inv_inertia_local = (C.c_float * 9)(*ii)
        _ffi.check(self.lib, self.lib.wgs_set_body_mass_properties(self._h, mp, n))

    def read_body_poses(self):
        """poses_staging read-back (src_testbed/step.rs:129-132): one dict per collider with rotation
        (3D quaternion (i,j,k,w); 2D (cos, sin)), translation, linvel, angvel, com as float64 arrays.
        Every rank of a sharded run integrates the same bodies, so any rank can be asked."""
        n, D = self.n_colliders, self.dim
        poses = (self.T.Pose * max(1, n))()
        vels = (self.T.Velocity * max(1, n))()
        coms = (C.c_float * (3 * max(1, n)))()
        _ffi.check(self.lib, self.lib.wgs_read_body_poses(self._h, poses, vels, coms, n))
        out = []
        for i in range(n):
            out.append(dict(rotation=np.array(list(poses[i].rotation)[:(2 if D == 2 else 4)], np.float64),
                            translation=np.array(list(poses[i].translation)[:D], np.float64),
                            linvel=np.array(list(vels[i].linear)[:D], np.float64),
                            angvel=np.array(list(vels[i].angular)[:(1 if D == 2 else 3)], np.float64),
                            com=np.array([coms[3 * i + k] for k in range(D)], np.float64)))
        return out

    # -- device -> host
    def sync(self):
        _ffi.check(self.lib, self.lib.wgs_sync(self._h))

    def diagnostics(self, what: int = _ffi.DIAG_PARTICLES) -> Diagnostics:
        """`wgs_read_diagnostics`: reproducible sums, bounds and the state digest of the state after the last enqueued substep,
        reduced on the device (blocking; nothing but the small struct crosses PCIe). `what` = OR of _ffi.DIAG_*.
        On a slab: over the slots this rank holds; counts, digests and `fixed` sums of equal exponent of the ranks add exactly, and
        combining them is the caller's task."""
        return read_diagnostics(self.lib, self._h, self.dim, what)

    def read_grid(self):
        """(cells[int32 M x D], vel_mass[M x (D+1)], cdf_dist, cdf_aff, cdf_closest), lexicographically
        sorted by cell coordinate (physical node ids are not comparable between runs). On a slab: the nodes of its own grid."""
        T, D = self.T, self.dim
        cnt = C.c_size_t(0)
        _ffi.check(self.lib, self.lib.wgs_read_grid(self._h, None, 0, C.byref(cnt)))
        m = cnt.value
        words = C.sizeof(T.NodeRecord) // 4
        raw = np.zeros((max(m, 1), words), np.int32)
        if m:
            _ffi.check(self.lib, self.lib.wgs_read_grid(self._h, raw.ctypes.data_as(C.POINTER(T.NodeRecord)), m, C.byref(cnt)))
        raw = raw[:m]
        cells = raw[:, :D].copy()
        fl = raw.view(F32)
        vm = fl[:, D:2 * D + 1].copy()
        dist = fl[:, 2 * D + 1].copy()
        aff = raw.view(np.uint32)[:, 2 * D + 2].copy()
        closest = raw.view(np.uint32)[:, 2 * D + 3].copy()
        order = np.lexsort(cells.T[::-1]) if m else np.zeros(0, np.int64)
        return cells[order], vm[order], dist[order], aff[order], closest[order]

    def enqueue_diagnostics(self, device_ptr: int, what: int = _ffi.DIAG_PARTICLES):
        """`wgs_enqueue_diagnostics`: the same, stream-ordered; the struct (`ctypes.sizeof(_ffi.Diagnostics)` bytes) is left at the
        DEVICE address `device_ptr`. Returns at once."""
        _ffi.check(self.lib, self.lib.wgs_enqueue_diagnostics(self._h, int(what), C.c_void_p(int(device_ptr))))

    def stats(self):
        s = self.T.Stats()
        _ffi.check(self.lib, self.lib.wgs_get_stats(self._h, C.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in s._fields_}

    def close(self):
        if getattr(self, "_h", None):
            self.lib.wgs_data_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MpmData(DataHandle):
    """src/pipeline.rs:84-173. Owns every device buffer of one simulation."""

    def __init__(self, pipeline: MpmPipeline, params: SimulationParams, particles: ParticleSet,
                 colliders: Sequence[Collider], cell_width: float, grid_capacity: int,
                 model: int = MODEL_COROTATED, particle_capacity: Optional[int] = None):
        super().__init__(pipeline, colliders)
        if particles.dim != self.dim:
            raise ValueError("particle dimension does not match the pipeline")
        self._n_static, self._emitting, self._num_sinks = particles.n, False, 0
        raw = _pack_particles(self.T, particles)
        h = C.c_void_p()
        args = (pipeline._h, C.byref(self._sim_params(params)), raw.ctypes.data_as(C.POINTER(self.T.Particle)), particles.n,
                self._collider_array(colliders), len(colliders), float(cell_width), int(grid_capacity))
        if particle_capacity is None:
            _ffi.check(self.lib, self.lib.wgs_data_create(*args, C.byref(h)))
        else:   # room for particles added at run time (add_particles, set_emitters)
            if int(particle_capacity) != particle_capacity or not 0 <= int(particle_capacity) < 2 ** 32:
                raise ValueError("particle_capacity is an unsigned 32-bit integer")
            _ffi.check(self.lib, self.lib.wgs_data_create_reserved(*args, int(particle_capacity), C.byref(h)))
        self._h = h
        if model != MODEL_COROTATED:
            self.set_constitutive_model(model)
        if any(_is_dynamic(c) for c in colliders):
            self.set_body_mass_properties(colliders)
        self._set_mesh_samples(colliders, cell_width)

    @classmethod
    def new(cls, pipeline, params, particles, colliders, cell_width, grid_capacity, model=MODEL_COROTATED, particle_capacity=None):
        """MpmData::new(device, params, &particles, &bodies, &colliders, cell_width, grid_capacity)
        (src/pipeline.rs:98-128). `particles` may be a ParticleSet or a list of Particle. `particle_capacity`: room for that many
        particles in all (`wgs_data_create_reserved`), to be filled by `add_particles` or emitters."""
        if not isinstance(particles, ParticleSet):
            particles = ParticleSet.from_particles(particles)
        return cls(pipeline, params, particles, colliders, cell_width, grid_capacity, model, particle_capacity)

    @property
    def n(self) -> int:
        """Particles the data holds now: those it was created with, those added and those its emitters emitted, less those removed and
        those its sinks took (host arithmetic on the library's counters: `stats()["num_particles"]` without its wait for the stream)."""
        return self._n_static + (sum(self.emitter_counts()[0]) if self._emitting else 0) - (sum(self.sink_counts()) if self._num_sinks else 0)

    def _rebase_n(self, n_now: int):
        """after a setter zeroed counters: `n` answers `n_now` again"""
        self._n_static = n_now
        self._n_static += n_now - self.n

    @property
    def particle_capacity(self) -> int:
        """`wgs_get_particle_capacity`: the particle slots reserved at creation."""
        cap = C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_get_particle_capacity(self._h, C.byref(cap)))
        return int(cap.value)

    def add_particles(self, particles: ParticleSet, models=None):
        """`wgs_add_particles`: `particles` behind the ones the data holds, with the caller's indices n .. n + k - 1; every reader
        includes them at once, and the next substep rebuilds the block table. `models`: one MODEL_* per new particle (np.uint8), read
        only while the data carries a per-particle table (None: the data's model). Needs room (`particle_capacity`). Blocking."""
        if particles.dim != self.dim:
            raise ValueError("particle dimension does not match the pipeline")
        raw = _pack_particles(self.T, particles)
        m = None
        if models is not None:
            m = np.ascontiguousarray(models, np.uint8).reshape(-1)
            if m.shape[0] != particles.n:
                raise ValueError("add_particles: one model per new particle")
        _ffi.check(self.lib, self.lib.wgs_add_particles(self._h, raw.ctypes.data_as(C.POINTER(self.T.Particle)),
                                                       m.ctypes.data_as(C.POINTER(C.c_uint8)) if m is not None else None, particles.n))
        self._n_static += particles.n

    def set_emitters(self, emitters):
        """`wgs_set_emitters`: up to `models.MAX_EMITTERS` `models.Emitter`, fired in this order in front of the substeps their schedule
        names, inside `MpmPipeline.step`; `None` or an empty list removes them. Replaces the whole set and zeroes `emitter_counts`.
        Host state of the handle: no device memory, not part of a checkpoint."""
        emitters = [] if emitters is None else list(emitters)
        E = _ffi.emitter_type(self.T, self.dim)
        arr = (E * max(len(emitters), 1))()
        for a, e in zip(arr, emitters):
            if e.proto.dim != self.dim:
                raise ValueError("set_emitters: the proto's dimension does not match the pipeline")
            words = _pack_particles(self.T, e.proto)
            C.memmove(C.byref(a.proto), words.ctypes.data, C.sizeof(self.T.Particle))
            a.model, a.spacing, a.jitter, a.seed = int(e.model), float(e.spacing), float(e.jitter), int(e.seed)
            a.lo[:] = [float(x) for x in e.lo]
            a.count[:] = [int(c) for c in e.count]
            a.start_substep, a.period, a.batches = int(e.start_substep), int(e.period), int(e.batches)
        n_now = self.n
        _ffi.check(self.lib, self.lib.wgs_set_emitters(self._h, arr if emitters else None, len(emitters)))
        self._emitting = bool(emitters)
        self._rebase_n(n_now)   # (the call zeroed the counters)

    def emitters(self):
        """`wgs_get_emitters`: what `set_emitters` last took, as `models.Emitter`."""
        from .models import Emitter
        E = _ffi.emitter_type(self.T, self.dim)
        arr = (E * _ffi.MAX_EMITTERS)()
        n = C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_get_emitters(self._h, arr, C.byref(n)))
        out = []
        for a in arr[:n.value]:
            words = np.frombuffer(bytes(a.proto), F32).reshape(1, -1).copy()
            out.append(Emitter(_unpack_particles(self.T, words, self.dim, None), tuple(a.lo), tuple(a.count), float(a.spacing), int(a.model),
                               float(a.jitter), int(a.seed), int(a.start_substep), int(a.period), int(a.batches)))
        return out

    def emitter_counts(self):
        """`wgs_get_emitter_counts`: (particles emitted, batches skipped for lack of room) per emitter of the set, as two lists."""
        emitted, skipped = (C.c_uint64 * _ffi.MAX_EMITTERS)(), (C.c_uint64 * _ffi.MAX_EMITTERS)()
        _ffi.check(self.lib, self.lib.wgs_get_emitter_counts(self._h, emitted, skipped))
        k = len(self.emitters()) if self._emitting else 0
        return [int(x) for x in emitted[:k]], [int(x) for x in skipped[:k]]

    def _removed(self, kept_from, removed: int, n_old: int):
        self._n_static -= removed
        return kept_from[:n_old - removed].copy()

    def remove_particles(self, mask):
        """`wgs_remove_particles`: `mask` has one entry per particle in the caller's order, nonzero (True) = remove. The survivors keep
        their relative order and are renumbered densely; every reader answers them under the new indices at once, and the next
        substep rebuilds the block table. Returns `kept_from` (np.uint32): the old index of every new index, for the caller's own
        per-particle arrays (`mine = mine[kept_from]`). Blocking: the new particle count is read back."""
        n_old = self.n
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, np.uint8)
        if m.shape[0] != n_old:
            raise ValueError("remove_particles: one mask entry per particle")
        kept_from, removed = np.zeros(max(n_old, 1), np.uint32), C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_remove_particles(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                          kept_from.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(removed)))
        return self._removed(kept_from, int(removed.value), n_old)

    def remove_particles_device(self, mask_ptr: int, kept_from_ptr: int = 0) -> int:
        """`wgs_remove_particles_device`: the same with the mask (one byte per particle) and, if wanted, `kept_from` (room for the old
        particle count, uint32) in device memory, read and written on the data's stream. Returns the number removed. Blocking."""
        removed = C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_remove_particles_device(self._h, C.c_void_p(int(mask_ptr)), C.c_void_p(int(kept_from_ptr)) if kept_from_ptr else None,
                                                                 C.byref(removed)))
        self._n_static -= int(removed.value)
        return int(removed.value)

    @staticmethod
    def _sink_array(sinks):
        sinks = [] if sinks is None else list(sinks)
        arr = (_ffi.Sink * max(len(sinks), 1))()
        for a, k in zip(arr, sinks):
            a.region, a.side, a.start_substep, a.period = int(k.region), int(k.side), int(k.start_substep), int(k.period)
            a.center[:] = [float(x) for x in k.center]
            a.half[:] = [float(x) for x in k.half]
        return sinks, arr

    def remove_particles_in(self, sinks):
        """`wgs_remove_particles_in`: the regions of up to `models.MAX_SINKS` `models.Sink` evaluated on the device, once, now (their
        schedule is ignored); otherwise `remove_particles`. Returns `kept_from`."""
        sinks, arr = self._sink_array(sinks)
        n_old = self.n
        kept_from, removed = np.zeros(max(n_old, 1), np.uint32), C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_remove_particles_in(self._h, arr if sinks else None, len(sinks),
                                                             kept_from.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(removed)))
        return self._removed(kept_from, int(removed.value), n_old)

    def set_sinks(self, sinks):
        """`wgs_set_sinks`: up to `models.MAX_SINKS` `models.Sink`, evaluated in one pass in front of the substeps their schedule names,
        ahead of the emitters, inside `MpmPipeline.step` — which then waits for the stream in front of those substeps; `None` or an empty
        list removes them. Replaces the whole set and zeroes `sink_counts`. Host state of the handle: no device memory, not part of a
        checkpoint."""
        sinks, arr = self._sink_array(sinks)
        n_now = self.n
        _ffi.check(self.lib, self.lib.wgs_set_sinks(self._h, arr if sinks else None, len(sinks)))
        self._num_sinks = len(sinks)
        self._rebase_n(n_now)   # (the call zeroed the sinks' counters, not the emitters')

    def sinks(self):
        """`wgs_get_sinks`: what `set_sinks` last took, as `models.Sink`."""
        from .models import Sink
        arr = (_ffi.Sink * _ffi.MAX_SINKS)()
        n = C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_get_sinks(self._h, arr, C.byref(n)))
        return [Sink(int(a.region), int(a.side), tuple(a.center), tuple(a.half), int(a.start_substep), int(a.period)) for a in arr[:n.value]]

    def sink_counts(self):
        """`wgs_get_sink_counts`: particles removed per sink of the set (a particle in several counts for the first), as a list."""
        removed = (C.c_uint64 * _ffi.MAX_SINKS)()
        _ffi.check(self.lib, self.lib.wgs_get_sink_counts(self._h, removed))
        return [int(x) for x in removed[:self._num_sinks]]

    @classmethod
    def from_scene(cls, pipeline, scene, **overrides):
        """The data one of the dicts `wgsparkl_amd.scenes` returns describes (the key table in that module's docstring): `new` with
        its "model" and "particle_capacity", then its "plasticity", "fluid_gamma", "models", "walls", "forces", "emitters" and "sinks" through their
        setters, in that order, each only where the scene has the key. A keyword replaces the scene's entry of that name for this call (`colliders=[]`, `grid_capacity=128`,
        `particles=snap`); `None` for one of the optional keys builds the scene without it (`models=None`: no table)."""
        sc = {"model": MODEL_COROTATED, **scene, **overrides}
        reserve = {} if sc.get("particle_capacity") is None else {"particle_capacity": sc["particle_capacity"]}
        data = cls.new(pipeline, sc["params"], sc["particles"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"], **reserve)
        for key, apply in (("plasticity", data.set_plasticity_model), ("fluid_gamma", data.set_fluid_eos),
                           ("models", data.set_particle_models), ("walls", data.set_domain_walls), ("forces", data.set_force_fields),
                           ("emitters", data.set_emitters), ("sinks", data.set_sinks)):
            if sc.get(key) is not None:
                apply(sc[key])
        return data

    def set_plasticity_model(self, kind: int):
        """`wgs_set_plasticity_model`: `models.PLASTICITY_DRUCKER_PRAGER` (default) or `models.PLASTICITY_SNOW` — the singular-value
        clamp with hardening on the corotated stress; the plasticity slots of a particle are then those of `models.Snow`.
        Stream-ordered; no device memory. MODEL_COROTATED data only."""
        _ffi.check(self.lib, self.lib.wgs_set_plasticity_model(self._h, int(kind)))

    def plasticity_model(self) -> int:
        """`wgs_get_plasticity_model`: the PLASTICITY_* value in force."""
        kind = C.c_int32(0)
        _ffi.check(self.lib, self.lib.wgs_get_plasticity_model(self._h, C.byref(kind)))
        return int(kind.value)

    def set_domain_walls(self, walls):
        """`wgs_set_domain_walls`: 2 * dim faces, `walls[2 * k]` the low face of axis k and `walls[2 * k + 1]` its high face, each a
        `models.Wall` (or a (type, friction, plane) triple) or None for no wall there; `None` for the whole list removes all walls.
        The nodes inside a face have their velocity projected after the grid update. Stream-ordered; no device memory."""
        if walls is None:
            _ffi.check(self.lib, self.lib.wgs_set_domain_walls(self._h, None))
            return
        walls = list(walls)
        if len(walls) != 2 * self.dim:
            raise ValueError("set_domain_walls: 2 * dim entries (low and high face of every axis)")
        arr = (_ffi.Wall * (2 * self.dim))()
        for f, w in enumerate(walls):
            if w is None:
                continue
            t, fr, pl = (w.type, w.friction, w.plane) if hasattr(w, "plane") else w
            if int(t) < 0 or int(pl) != pl:
                raise ValueError("set_domain_walls: type is a WALL_* value, plane an integer")
            arr[f].type, arr[f].friction, arr[f].plane = int(t), float(fr), int(pl)
        _ffi.check(self.lib, self.lib.wgs_set_domain_walls(self._h, arr))

    def domain_walls(self):
        """`wgs_get_domain_walls`: the 2 * dim faces as `models.Wall` (type WALL_NONE where there is none)."""
        from .models import Wall
        arr = (_ffi.Wall * (2 * self.dim))()
        _ffi.check(self.lib, self.lib.wgs_get_domain_walls(self._h, arr))
        return [Wall(int(w.type), float(w.friction), int(w.plane)) for w in arr]

    def set_force_fields(self, fields):
        """`wgs_set_force_fields`: up to `models.MAX_FORCE_FIELDS` `models.ForceField` (uniform, radial, vortex, drag; each everywhere, in a
        box or in a ball), applied to the grid nodes' velocities in this order once per substep, behind the grid update and in front of
        the domain walls; an entry None is kept as a FORCE_NONE entry and skipped; `None` or an empty list removes every field.
        Stream-ordered; no device memory; not part of a checkpoint."""
        fields = [] if fields is None else list(fields)
        arr = (_ffi.ForceField * max(len(fields), 1))()
        for a, f in zip(arr, fields):
            if f is None:
                continue
            a.kind, a.falloff, a.region = int(f.kind), int(f.falloff), int(f.region)
            a.strength, a.softening = float(f.strength), float(f.softening)
            for name in ("center", "vec", "region_center", "region_half"):
                v = tuple(getattr(f, name))
                getattr(a, name)[:] = [float(x) for x in v + (0.0,) * (3 - len(v))]
        _ffi.check(self.lib, self.lib.wgs_set_force_fields(self._h, arr if fields else None, len(fields)))

    def force_fields(self):
        """`wgs_get_force_fields`: what `set_force_fields` last took, as `models.ForceField` (FORCE_NONE entries included)."""
        from .models import ForceField
        arr = (_ffi.ForceField * _ffi.MAX_FORCE_FIELDS)()
        n = C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_get_force_fields(self._h, arr, C.byref(n)))
        return [ForceField(int(a.kind), int(a.falloff), int(a.region), float(a.strength), float(a.softening), tuple(a.center), tuple(a.vec),
                           tuple(a.region_center), tuple(a.region_half)) for a in arr[:n.value]]

    def set_particle_models(self, models):
        """`wgs_set_particle_models`: one MODEL_COROTATED / MODEL_NEO_HOOKEAN / MODEL_FLUID per particle (np.uint8, the caller's order) —
        fluid and solids in one simulation, coupled through the grid. `None` drops the table. Blocking."""
        if models is None:
            _ffi.check(self.lib, self.lib.wgs_set_particle_models(self._h, None))
            return
        m = np.ascontiguousarray(models, np.uint8).reshape(-1)
        if m.shape[0] != self.n:
            raise ValueError("set_particle_models: one entry per particle")
        _ffi.check(self.lib, self.lib.wgs_set_particle_models(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def read_particle_models(self) -> np.ndarray:
        """`wgs_read_particle_models`: the model of every particle in the caller's order (np.uint8); the data's model without a table."""
        out = np.zeros(self.n, np.uint8)
        _ffi.check(self.lib, self.lib.wgs_read_particle_models(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def read_positions(self) -> np.ndarray:
        out = np.zeros((self.n, self.dim), F32)
        _ffi.check(self.lib, self.lib.wgs_read_positions(self._h, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def device_ptrs(self):
        """`wgs_get_device_ptrs`: where the current particle state lives on the device (position quads + particle ids in
        sorted order, and the HIP stream that produces them) — the optional interop view, for readers on the same device."""
        v = _ffi.DevicePtrs()
        _ffi.check(self.lib, self.lib.wgs_get_device_ptrs(self._h, C.byref(v)))
        return v

    def read_particles(self) -> ParticleSet:
        T = self.T
        words = C.sizeof(T.Particle) // 4
        raw = np.zeros((self.n, words), F32)
        plastic = np.zeros((self.n, 3), F32)
        _ffi.check(self.lib, self.lib.wgs_read_particles(
            self._h, raw.ctypes.data_as(C.POINTER(T.Particle)), plastic.ctypes.data_as(C.POINTER(T.PlasticState))))
        return _unpack_particles(T, raw, self.dim, plastic)

    def prep_vertex_buffer(self, mode: int = 0, base_color=None) -> np.ndarray:
        """src_testbed/prep_vertex_buffer{2,3}d.wgsl: n x 24 floats (deformation 3 x vec4, position vec4, base_color,
        color), particle i of the caller's order in row i. `base_color`: n x 4 (default opaque white)."""
        inst = np.zeros((self.n, 24), F32)
        inst[:, 16:20] = 1.0 if base_color is None else np.asarray(base_color, F32).reshape(self.n, 4)
        _ffi.check(self.lib, self.lib.wgs_prep_vertex_buffer(self._h, int(mode), inst.ctypes.data_as(C.c_void_p)))
        return inst

    def set_plastic_state(self, dp_state: np.ndarray):
        """Checkpoint restore of the Drucker-Prager plastic state (n x 3: plastic det, hardening, log_vol_gain)
        in the caller's particle order; together with `MpmData.new(read_particles())` it continues a run
        bit-exactly."""
        st = np.ascontiguousarray(dp_state, F32).reshape(self.n, 3)
        _ffi.check(self.lib, self.lib.wgs_set_plastic_state(self._h, st.ctypes.data_as(C.POINTER(self.T.PlasticState))))

    def read_blocks(self, with_sorted_ids: bool = True):
        """(vid, first_particle, num_particles) sorted by vid, and sorted particle ids."""
        T, D = self.T, self.dim
        cnt = C.c_size_t(0)
        _ffi.check(self.lib, self.lib.wgs_read_blocks(self._h, None, 0, C.byref(cnt), None))
        m = cnt.value
        raw = np.zeros((max(m, 1), D + 2), np.int32)
        ids = np.zeros(max(self.n, 1), np.uint32)
        _ffi.check(self.lib, self.lib.wgs_read_blocks(
            self._h, raw.ctypes.data_as(C.POINTER(T.BlockRecord)), m, C.byref(cnt),
            ids.ctypes.data_as(C.POINTER(C.c_uint32)) if with_sorted_ids else None))
        raw = raw[:m]
        vid = raw[:, :D].copy()
        order = np.lexsort(vid.T[::-1]) if m else np.zeros(0, np.int64)
        u = raw.view(np.uint32)
        return vid[order], u[:, D][order].copy(), u[:, D + 1][order].copy(), ids[:self.n]

    # -- Lagrangian field output: stress and strain of every particle's stored state, evaluated on the device
    def particle_fields(self) -> ParticleFields:
        """`wgs_read_particle_fields`: Kirchhoff stress, mean stress, von Mises stress, volume ratio, stretches and model of every
        particle, in the caller's order, with the step's own constitutive functions. Blocking; writes no state."""
        words = np.zeros((self.n, C.sizeof(self.T.ParticleField) // 4), np.uint32)
        _ffi.check(self.lib, self.lib.wgs_read_particle_fields(self._h, words.ctypes.data_as(C.POINTER(self.T.ParticleField))))
        return particle_fields_from_words(words, self.dim)

    def particle_fields_device(self, out_ptr: int):
        """`wgs_read_particle_fields_device`: the same into DEVICE memory (`out_ptr`: n records of `ctypes.sizeof(T.ParticleField)`
        bytes, aligned to 16 bytes), stream-ordered on the data's stream. Returns at once."""
        _ffi.check(self.lib, self.lib.wgs_read_particle_fields_device(self._h, C.c_void_p(int(out_ptr))))

    # -- Eulerian field output: the grid of the last substep at arbitrary points, and a dense window of its nodes
    def sample_grid(self, points) -> GridSamples:
        """`wgs_sample_grid`: velocity, velocity gradient, density and the number of active stencil nodes at every row of `points`
        [n, D], with the step's own stencil on the grid `read_grid` reports. Blocking."""
        D = self.dim
        pts = np.ascontiguousarray(points, F32).reshape(-1, D)
        n = pts.shape[0]
        words = np.zeros((n, C.sizeof(self.T.GridSample) // 4), np.uint32)
        _ffi.check(self.lib, self.lib.wgs_sample_grid(self._h, pts.ctypes.data_as(C.POINTER(C.c_float)), n,
                                                      words.ctypes.data_as(C.POINTER(self.T.GridSample))))
        return grid_samples_from_words(words, D)

    def sample_grid_device(self, points_ptr: int, n: int, out_ptr: int):
        """`wgs_sample_grid_device`: the same on DEVICE memory (`points_ptr`: n * D floats, `out_ptr`: n records of
        `ctypes.sizeof(T.GridSample)` bytes), stream-ordered on the data's stream. Returns at once."""
        _ffi.check(self.lib, self.lib.wgs_sample_grid_device(self._h, C.c_void_p(int(points_ptr)), int(n), C.c_void_p(int(out_ptr))))

    def _window_args(self, lo, dims):
        D = self.dim
        lo = np.ascontiguousarray(lo, np.int32).reshape(D)
        dims = np.ascontiguousarray(dims, np.uint32).reshape(D)
        return lo, dims, lo.ctypes.data_as(C.POINTER(C.c_int32)), dims.ctypes.data_as(C.POINTER(C.c_uint32))

    def grid_window(self, lo, dims):
        """`wgs_read_grid_window`: (velocity[dims..., D], mass[dims...]) of the world cells lo + (i, j[, k]), the x index first; the raw
        node values of `read_grid`, +0 outside the active blocks. Blocking."""
        D = self.dim
        lo, dims, plo, pdims = self._window_args(lo, dims)
        total = int(np.prod(dims.astype(np.uint64)))
        ok = bool(np.all(dims >= 1)) and total < 2 ** 31
        out = np.zeros((total if ok else 1) * (D + 1), F32)    # (a refused call writes nothing)
        _ffi.check(self.lib, self.lib.wgs_read_grid_window(self._h, plo, pdims, out.ctypes.data_as(C.POINTER(C.c_float))))
        nodes = out.reshape(tuple(int(x) for x in dims[::-1]) + (D + 1,))          # stored with x fastest
        nodes = nodes.transpose(tuple(range(D - 1, -1, -1)) + (D,))
        return nodes[..., :D].copy(), nodes[..., D].copy()

    def grid_window_device(self, lo, dims, out_ptr: int):
        """`wgs_read_grid_window_device`: the same into DEVICE memory (prod(dims) * (D + 1) floats, x fastest), stream-ordered on the
        data's stream. Returns at once."""
        lo, dims, plo, pdims = self._window_args(lo, dims)
        _ffi.check(self.lib, self.lib.wgs_read_grid_window_device(self._h, plo, pdims, C.c_void_p(int(out_ptr))))

    def read_timings(self):
        ms = (C.c_float * _ffi.WGS_NUM_PASSES)()
        _ffi.check(self.lib, self.lib.wgs_read_timings(self._h, ms))
        return dict(zip(_ffi.PASS_NAMES, [float(x) for x in ms]))
