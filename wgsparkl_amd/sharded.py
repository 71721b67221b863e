"""Multi-GPU host glue: x-slab domain decomposition of the MLS-MPM substep, one process per GPU.

NEW DESIGN — the reference is single-GPU (one wgpu::Device, src/pipeline.rs:176-193).
The substep protocol itself lives in the library (include/wgsparkl_hip.h "Multi-GPU": `wgs_comm_*`, `wgs_shard_attach`,
`wgs_sharded_step`; wgsparkl_amd/csrc/kernels_shard.h, capi_sharded.inc) — ONE implementation, in C++, RCCL
point-to-point as its transport. This module only holds what a host needs around it: the partition of block space into
slabs, thin ctypes wrappers of a communicator and a slab, and the record layout of `wgs_shard_export`.

Why x slabs and what crosses a face: a particle with associated cell c touches nodes c..c+2 only, so a rank's particles
reach the first two node layers of the block layer owned by the NEXT rank and nothing on the lower side. Per substep ONE
message per neighbour: the partial (momentum, mass) sums of the node layers the two ranks share (both add what they
receive: a + b == b + a bitwise, so both hold identical totals and update them redundantly) and, in the same message,
the records of the particles that changed owner in the previous substep — the old owner still transfers them to the
grid, the new owner advances them (kernels_shard.h). A slab with two neighbours must be at least 3 blocks wide.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _ffi
from .models import MODEL_COROTATED
from .pipeline import DataHandle, MpmPipeline, _is_dynamic, _pack_particles
from .solver import ParticleSet, SimulationParams

INT_MIN, INT_MAX = -(2 ** 31), 2 ** 31 - 1
MIN_INTERIOR_WIDTH = 3      # blocks; wgs_shard_attach refuses narrower slabs between two neighbours


@dataclass
class SlabPartition:
    """Contiguous block ranges along x: rank r owns bx in [cuts[r], cuts[r+1]); the two ends are open."""
    cuts: Sequence[int]          # world + 1 entries, in BLOCK units (4 cells in 3D, 8 in 2D)

    @property
    def world(self) -> int:
        return len(self.cuts) - 1

    def block_range(self, rank: int):
        lo = INT_MIN if rank == 0 else int(self.cuts[rank])
        hi = INT_MAX if rank == self.world - 1 else int(self.cuts[rank + 1])
        return lo, hi

    def owner_of_blocks(self, bx: np.ndarray) -> np.ndarray:
        inner = np.asarray(self.cuts[1:-1], np.int64)
        return np.searchsorted(inner, np.asarray(bx, np.int64), side="right")

    @staticmethod
    def balanced(block_x: np.ndarray, world: int) -> "SlabPartition":
        """Cuts at particle-count quantiles of the associated block x coordinate (balance by particle
        count, not by volume)."""
        bx = np.sort(np.asarray(block_x, np.int64))
        cuts = [int(bx[0])]
        for r in range(1, world):
            cuts.append(int(bx[(len(bx) * r) // world]))
        cuts.append(int(bx[-1]) + 1)
        for i in range(1, len(cuts)):          # strictly increasing; interior slabs wide enough for the protocol
            cuts[i] = max(cuts[i], cuts[i - 1] + (MIN_INTERIOR_WIDTH if 1 < i < len(cuts) - 1 else 1))
        return SlabPartition(cuts)

    def min_interior_width(self) -> int:
        """Narrowest slab that has two neighbours (blocks); a large number when there is none."""
        w = [self.cuts[r + 1] - self.cuts[r] for r in range(1, self.world - 1)]
        return int(min(w)) if w else 1 << 30


def associated_block_x(pos: np.ndarray, cell_width: float, dim: int) -> np.ndarray:
    """floor((round(x / h) - 1) / BW) with the reference's fp32 rule (particle3d.wgsl:41-49, grid.wgsl:284-292)."""
    bw = 4 if dim == 3 else 8
    c = np.rint(pos[:, 0].astype(np.float32) / np.float32(cell_width)) - np.float32(1.0)
    return np.floor(c / np.float32(bw)).astype(np.int64)


# ------------------------------------------------------------------------------------------------
# The substep driven from inside the library (include/wgsparkl_hip.h: wgs_comm_*, wgs_shard_attach,
# wgs_sharded_step): what bench.py --gpus N and a Rust caller use.
# ------------------------------------------------------------------------------------------------
class NativeComm:
    """RCCL communicator owned by the library (`wgs_comm_create`). The 128-byte unique id is made by rank 0 and
    handed around with whatever the host has — here torch.distributed's broadcast."""

    def __init__(self, pipeline: MpmPipeline, dist, rank: int, world: int, flags: int = 0):
        import torch
        self.lib, self.rank, self.world = pipeline.lib, rank, world
        uid = C.create_string_buffer(128)
        failure = None
        if rank == 0:
            try:
                _ffi.check(self.lib, self.lib.wgs_comm_get_unique_id(uid))
            except Exception as e:  # noqa: BLE001 — the other ranks are waiting in the broadcast below: send them zeros
                failure = e
                uid = C.create_string_buffer(128)
        if world > 1:
            t = torch.tensor(list(uid.raw), dtype=torch.uint8)
            if dist.get_backend() == "nccl":
                t = t.to(torch.device("cuda", pipeline.device))
            dist.broadcast(t, 0)
            uid = C.create_string_buffer(bytes(t.cpu().numpy().tobytes()), 128)
        if failure is not None or not any(uid.raw):
            raise RuntimeError(f"no RCCL unique id from rank 0 ({failure})")   # on every rank alike
        h = C.c_void_p()
        _ffi.check(self.lib, self.lib.wgs_comm_create(pipeline._h, uid, rank, world, int(flags), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.wgs_comm_destroy(self._h)
            self._h = None


class NativeShard(DataHandle):
    """One slab as a Rust caller would hold it: a sharded `wgs_data` whose message buffers and substep protocol live
    in the library. `comm` = NativeComm (one process per GPU) or None (a slab of a lockstep group / no neighbours)."""

    def __init__(self, pipeline: MpmPipeline, params: SimulationParams, particles: ParticleSet, global_ids: np.ndarray,
                 colliders, cell_width: float, grid_capacity: int, block_lo: int, block_hi: int, has_lower: bool,
                 has_upper: bool, particle_capacity: int, model: int = MODEL_COROTATED, force_plastic: bool = False,
                 halo_capacity_records: int = 4096, migrant_capacity: int = 4096, comm: Optional[NativeComm] = None,
                 uniform_material=None):
        """`uniform_material` = (mass, init_volume, lambda, mu) shared by EVERY particle of EVERY rank (the caller's
        promise: a rank only sees its own), or None: the constants then travel with each particle."""
        super().__init__(pipeline, colliders)
        self.uniform_material = uniform_material
        raw = _pack_particles(self.T, particles)
        gids = np.ascontiguousarray(global_ids, np.uint32)
        h = C.c_void_p()
        cap = max(int(particle_capacity), particles.n)
        _ffi.check(self.lib, self.lib.wgs_data_create_sharded(
            pipeline._h, C.byref(self._sim_params(params)), raw.ctypes.data_as(C.POINTER(self.T.Particle)), particles.n,
            gids.ctypes.data_as(C.POINTER(C.c_uint32)), self._collider_array(colliders), len(colliders), float(cell_width),
            int(grid_capacity), cap, max(int(block_lo), INT_MIN), min(int(block_hi), INT_MAX), 1 if force_plastic else 0, C.byref(h)))
        self._h = h
        self.capacity = cap
        if model != MODEL_COROTATED:
            self.set_constitutive_model(model)
        if uniform_material is not None:
            _ffi.check(self.lib, self.lib.wgs_set_uniform_material(self._h, *[float(x) for x in uniform_material]))
            self.sync()                                            # (a particle with other constants is reported here)
        if any(_is_dynamic(c) for c in colliders):                 # dynamic bodies: two-way coupling
            self.set_body_mass_properties(colliders)
        _ffi.check(self.lib, self.lib.wgs_shard_attach(self._h, comm._h if comm is not None else None, 1 if has_lower else 0,
                                                         1 if has_upper else 0, int(halo_capacity_records), int(migrant_capacity)))
        self._set_mesh_samples(colliders, cell_width)              # every rank holds every sample
        self.part_rec = self.lib.wgs_shard_particle_record_bytes() // 4
        self.hdr = self.lib.wgs_shard_buffer_header_bytes() // 4

    @classmethod
    def from_scene(cls, pipeline: MpmPipeline, slab_scene, rank: int, comm: Optional[NativeComm] = None, particle_capacity: int = 0,
                   force_plastic: bool = False, halo_capacity_records: int = 4096, migrant_capacity: int = 4096, **overrides):
        """The slab of `rank` from a slab scene (the key table in the docstring of `wgsparkl_amd.scenes`): its block range and
        its neighbours from the scene's "partition", its "global_ids", "model" and "uniform_material", then its "fluid_gamma".
        A keyword replaces the scene's entry of that name, as in `MpmData.from_scene`. "plasticity", "models", "walls", "forces",
        "emitters" and "sinks" are single-domain features the library refuses on a slab: a scene that holds one is an error unless the caller
        passes `plasticity=None` / `models=None` / `walls=None` / `forces=None` / `emitters=None` / `sinks=None`. `particle_capacity` = 0: room for the slab's
        own particles only — the argument is the slab's room for migrants; a SCENE's "particle_capacity" (its reservation for particles
        added at run time, which a slab cannot take) is refused like the other keys."""
        sc = {"model": MODEL_COROTATED, **slab_scene, **overrides}
        for key in ("plasticity", "models", "walls", "forces", "emitters", "sinks"):
            if sc.get(key) is not None:
                raise ValueError(f"NativeShard.from_scene: the scene's {key!r} cannot be applied to a slab; pass {key}=None to build it without")
        if slab_scene.get("particle_capacity") is not None:
            raise ValueError("NativeShard.from_scene: the scene's 'particle_capacity' (room for particles added at run time) cannot be applied "
                             "to a slab; build the slab scene without the key")
        part = sc["partition"]
        lo, hi = part.block_range(rank)
        shard = cls(pipeline, sc["params"], sc["particles"], sc["global_ids"], sc["colliders"], sc["cell_width"], sc["grid_capacity"],
                    lo, hi, rank > 0, rank < part.world - 1, particle_capacity, model=sc["model"], force_plastic=force_plastic,
                    halo_capacity_records=halo_capacity_records, migrant_capacity=migrant_capacity, comm=comm,
                    uniform_material=sc.get("uniform_material"))
        if sc.get("fluid_gamma") is not None:
            shard.set_fluid_eos(sc["fluid_gamma"])
        return shard

    def step(self, num_substeps: int):
        """`wgs_sharded_step`: whole substeps incl. the neighbour exchange, asynchronous."""
        _ffi.check(self.lib, self.lib.wgs_sharded_step(self.pipeline._h, self._h, int(num_substeps)))

    def num_particles(self) -> int:
        return self.stats()["num_particles"]

    def export_records(self) -> np.ndarray:
        """The exchange records of the particles this rank holds now, float32 [count, record_floats(dim)]: every quad of the
        particle, its global id and the substep its cdf was computed in (blocking). The one caller of `wgs_shard_export`."""
        import torch
        buf = torch.zeros(self.hdr + self.capacity * self.part_rec, dtype=torch.float32, device=torch.device("cuda", self.pipeline.device))
        # the library writes on its own non-blocking stream: torch's fill must be done first, or it can land on the export
        torch.cuda.current_stream(buf.device).synchronize()
        cnt = C.c_uint32(0)
        _ffi.check(self.lib, self.lib.wgs_shard_export(self._h, C.c_void_p(buf.data_ptr()), self.capacity, C.byref(cnt)))
        return buf[self.hdr: self.hdr + cnt.value * self.part_rec].cpu().numpy().reshape(cnt.value, self.part_rec)

    def export(self, cdf: bool = False, plastic: bool = False):
        """(global ids, pos, vel, def_grad, affine, mass) of the particles this rank owns now, with `cdf` also their cdf, with
        `plastic` also their plasticity parameters, plastic state and phase (`unpack_records`); blocking."""
        return unpack_records(self.export_records(), self.dim, self.uniform_material if self.dim == 3 else None, cdf, plastic)


def native_lockstep(pipeline: MpmPipeline, shards: List[NativeShard], num_substeps: int):
    """`wgs_sharded_step_lockstep`: all slabs of one process on one device, in x order."""
    arr = (C.c_void_p * len(shards))(*[s._h for s in shards])
    _ffi.check(pipeline.lib, pipeline.lib.wgs_sharded_step_lockstep(pipeline._h, arr, len(shards), int(num_substeps)))


def uniform_material_of(particles: ParticleSet):
    """(mass, init_volume, lambda, mu) if all particles of the set share them bitwise, else None."""
    if particles.n == 0:
        return None
    cols = (particles.mass, particles.init_volume, particles.lambda_, particles.mu)
    if all(bool(np.all(c.view(np.uint32) == c.view(np.uint32)[0])) for c in cols):
        return tuple(float(c[0]) for c in cols)
    return None


# The quads of a particle slot — and of an exchange record, which is a slot's quads followed by its id and the substep of
# its cdf — per dimension, under the names of Pl<D> in csrc/layout.h (tests/test_quad_table.py holds the two equal).
QUADS = {
    3: dict(XM=0, CV0=1, CV1=2, CV2=3, F0=4, F1=5, F2=6, NBASE=7, DP0=7, DP1=8, DP2=9, CDF0=10, CDF1=11, NQ=12),
    2: dict(XM=0, CV0=1, CV2=2, F0=3, NBASE=4, DP0=4, DP1=5, DP2=6, CDF0=7, CDF1=8, NQ=9),
}


def record_floats(dim: int) -> int:
    """floats per exchange record (csrc/kernels_shard.h particle_record_floats)"""
    return QUADS[dim]["NQ"] * 4 + 2


def record_quad(rec: np.ndarray, dim: int, name: str) -> np.ndarray:
    """the four floats of quad `name` of every record [count, 4] (a view)"""
    k = QUADS[dim][name]
    return rec[:, 4 * k:4 * k + 4]


def unpack_records(rec: np.ndarray, dim: int, uniform_material=None, cdf: bool = False, plastic: bool = False):
    """Particle records (quad layout of csrc/layout.h) -> dict of arrays. In uniform-material mode (3D) the record's
    XM.w slot holds F[8] and the mass is the shared one. `cdf`: also cdf_affinity, cdf_dist, cdf_normal and cdf_stamp, the
    substep the cdf was computed in. `plastic`: also dp [n, 6], dp_state [n, 3] and phase [n, 2] in the general layout of the
    DP quads, the only one a slab uses (layout.h: uni_dp is single-domain)."""
    ids = rec[:, -2].copy().view(np.uint32)     # [..quads.., pid, cdf epoch]
    q = lambda name: record_quad(rec, dim, name)
    if dim == 3:
        pos, mass = q("XM")[:, :3], q("XM")[:, 3]
        C_ = np.concatenate([q("CV0"), q("CV1"), q("CV2")[:, :1]], 1)
        vel = q("CV2")[:, 1:4]
        F = np.concatenate([q("F0"), q("F1"), q("F2")[:, :1]], 1)
        if uniform_material is not None:
            F = np.concatenate([q("F0"), q("F1"), q("XM")[:, 3:4]], 1)
            mass = np.full(len(rec), np.float32(uniform_material[0]), np.float32)
        aff, dist, normal = q("CDF1")[:, 3], q("CDF0")[:, 3], q("CDF0")[:, :3]
    else:
        pos, mass = q("XM")[:, :2], q("XM")[:, 2]
        C_, vel, F = q("CV0"), q("CV2")[:, :2], q("F0")
        aff, dist, normal = q("CDF0")[:, 3], q("CDF0")[:, 2], q("CDF0")[:, :2]
    out = dict(ids=ids, pos=pos.copy(), vel=vel.copy(), def_grad=F.copy(), affine=C_.copy(), mass=mass.copy())
    if cdf:
        out.update(cdf_affinity=aff.copy().view(np.uint32), cdf_dist=dist.copy(), cdf_normal=normal.copy(),
                   cdf_stamp=rec[:, -1].copy().view(np.uint32))
    if plastic:      # DP0 = h0..h3; DP1 = lambda, mu, plastic det, hardening; DP2 = log_vol_gain, phase, max_stretch, -
        out.update(dp=np.concatenate([q("DP0"), q("DP1")[:, :2]], 1), dp_state=np.concatenate([q("DP1")[:, 2:4], q("DP2")[:, :1]], 1),
                   phase=q("DP2")[:, 1:3].copy())
    return out


class JoinedSlabs(NamedTuple):
    """what join_slabs returns"""
    ids: np.ndarray              # the ids the slabs hold, ascending (int64)
    fields: dict                 # each field concatenated over the ranks, in the order of `ids`
    holder: np.ndarray           # the rank that holds each particle, in the same order
    counts: list                 # particles per rank
    exact: bool                  # the ids are the expected set, each once
    problem: str                 # the message of a failed `assert joined.exact`


def join_slabs(outs, ids=None, fields=None) -> JoinedSlabs:
    """The slabs of a decomposition as one domain, in the order of the global ids: a slab holds its particles in the order they
    arrived, so ids, never slots, are what two runs have in common. `outs`: one mapping per rank with an "ids" entry (`export()`
    dicts, a worker's saved arrays); `fields`: the per-particle entries to join (default: every key of the first mapping but
    "ids"); `ids`: the expected ids (default: 0 .. total - 1). Pure numpy; raises nothing: `exact` is the verdict."""
    fields = [k for k in outs[0].keys() if k != "ids"] if fields is None else fields
    counts = [int(len(o["ids"])) for o in outs]
    got = np.concatenate([o["ids"] for o in outs]).astype(np.int64)
    order = np.argsort(got, kind="stable")
    got = got[order]
    want = np.arange(len(got)) if ids is None else np.sort(np.asarray(ids, np.int64))
    uniq, times = np.unique(got, return_counts=True)
    problem = (f"every particle exactly once: per rank {counts}, missing {np.setdiff1d(want, uniq)[:20].tolist()}, "
               f"duplicated {uniq[times > 1][:20].tolist()}, unexpected {np.setdiff1d(uniq, want)[:20].tolist()}")
    return JoinedSlabs(got, {f: np.concatenate([o[f] for o in outs])[order] for f in fields},
                       np.concatenate([np.full(c, r) for r, c in enumerate(counts)])[order], counts, bool(np.array_equal(got, want)), problem)


def by_id(out):
    """One export with every entry in the order of ascending ids (stable): two slabs that hold the same particles compare
    entry by entry, whatever order their slots are in."""
    order = np.argsort(out["ids"], kind="stable")
    return {k: v[order] for k, v in out.items()}


def split_scene(particles: ParticleSet, partition: SlabPartition, cell_width: float):
    """Assign every particle to the rank owning its associated block; returns per-rank (ParticleSet, global ids)."""
    bx = associated_block_x(particles.pos, cell_width, particles.dim)
    owner = partition.owner_of_blocks(bx)
    out = []
    for r in range(partition.world):
        idx = np.nonzero(owner == r)[0]
        sub = ParticleSet(**{k: (v[idx] if isinstance(v, np.ndarray) else v) for k, v in particles.__dict__.items()})
        out.append((sub, idx.astype(np.uint32)))
    return out


def lockstep_slabs(pipeline: MpmPipeline, scene, world: int, part: Optional[SlabPartition] = None, **kw):
    """A whole scene cut into `world` x-slabs balanced by particle count (or by the given SlabPartition), each a NativeShard of a
    lockstep group (`native_lockstep`) with room for every particle of the scene; `kw` as in `NativeShard.from_scene`.
    Returns (shards, partition)."""
    ps = scene["particles"]
    part = part or SlabPartition.balanced(associated_block_x(ps.pos, scene["cell_width"], ps.dim), world)
    kw.setdefault("particle_capacity", ps.n)
    slab = {**scene, "partition": part, "uniform_material": uniform_material_of(ps)}
    return [NativeShard.from_scene(pipeline, {**slab, "particles": sub, "global_ids": gids}, r, **kw)
            for r, (sub, gids) in enumerate(split_scene(ps, part, scene["cell_width"]))], part
