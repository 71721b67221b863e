"""Synthetic scenes (the workloads of BASELINE.json / SURVEY.md §8d).

Conventions follow the reference's example scenes: lattice spacing h/2
(8 particles per cell in 3D, 4 in 2D), radius h/4, `with_density`
(crates/wgsparkl3d/examples/sand3.rs:28-49, crates/wgsparkl2d/examples/elasticity2.rs:33-55),
plus a reproducible jitter so cells are not degenerate.

The scene contract. Every builder returns a dict, and `MpmData.from_scene` (a whole scene) and `NativeShard.from_scene` /
`sharded.lockstep_slabs` (slabs) are the ones that read it:

| key | | what the constructors do with it |
|---|---|---|
| `particles`, `params`, `colliders`, `cell_width`, `grid_capacity` | required | the arguments of `MpmData.new` / `NativeShard` |
| `model` | optional | the data's single constitutive model; default `MODEL_COROTATED` |
| `plasticity` | optional | the plasticity rule, `PLASTICITY_DRUCKER_PRAGER` / `PLASTICITY_SNOW`: `MpmData.set_plasticity_model`; an error on a slab |
| `fluid_gamma` | optional | the Tait exponent of `MODEL_FLUID`: `set_fluid_eos` |
| `models` | optional | the per-particle table (np.uint8): `MpmData.set_particle_models`; an error on a slab |
| `walls` | optional | the 2 * dim domain walls: `MpmData.set_domain_walls`; an error on a slab |
| `forces` | optional | the force fields (a list of `models.ForceField`): `MpmData.set_force_fields`; an error on a slab |
| `particle_capacity` | optional | room for that many particles in all, to be filled at run time (`MpmData.add_particles`, emitters): `wgs_data_create_reserved`; an error on a slab |
| `emitters` | optional | the emitters (a list of `models.Emitter`): `MpmData.set_emitters`; an error on a slab |
| `sinks` | optional | the sinks (a list of `models.Sink`): `MpmData.set_sinks`; an error on a slab |
| `global_ids`, `partition` | slab scenes | the particles' names in the whole scene; the `SlabPartition` the slab's block range and neighbours come from |
| `uniform_material` | slab scenes, optional | (mass, init_volume, lambda, mu) shared by every particle of every rank |

The optional keys are applied at creation in the order of the table (`particle_capacity` with the creation itself), each only where
the scene has the key and its value is not None. Any other key (`fluid`, `solid_model`, `global_particles`, `name`, `bytes_per_particle`, ...) is information for the
caller; the constructors ignore it.
"""
from __future__ import annotations

import numpy as np

from .models import (MODEL_COROTATED, MODEL_FLUID, MODEL_NEO_HOOKEAN, PLASTICITY_DRUCKER_PRAGER, PLASTICITY_SNOW, WALL_SLIP, WALL_STICKY,
                     DruckerPrager, ElasticCoefficients, Emitter, FluidCoefficients, ForceField, ParticlePhase, Sink, Snow, Wall)
from .solver import SHAPE_CAPSULE, Collider, ParticleSet, SimulationParams

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def lattice(counts, origin, cell_width, jitter=0.05, seed=1234):
    """Particles at spacing h/2 starting at `origin` (+h/4), uniform jitter ±jitter*h."""
    dim = len(counts)
    axes = [np.arange(c, dtype=np.float64) for c in counts]
    grid = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, dim)
    pos = (grid + 0.5) * (cell_width / 2.0) + np.asarray(origin, np.float64)
    if jitter:
        rng = np.random.default_rng(seed)
        pos = pos + rng.uniform(-jitter * cell_width, jitter * cell_width, size=pos.shape)
    return pos.astype(F32)


def reference_smoke_scene():
    """The scene of the reference's own smoke tests (src/pipeline.rs:302-331,
    src/grid/grid.rs:355-370): 10^3 particles at i/2, r = h/4, rho = 1,
    E = 1e5, nu = 0.33, plasticity None, phase None (quirk B1), g = (0,-9.81,0),
    dt = 1/600, h = 1, no colliders, capacity 100_000."""
    h = 1.0
    idx = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    pos = (idx.astype(F32) / F32(h)) / F32(2.0)
    ps = ParticleSet.uniform(pos, h / 4.0, 1.0, ElasticCoefficients.from_young_modulus(100_000.0, 0.33))
    params = SimulationParams(gravity=(0.0, -9.81, 0.0), dt=float(F32(1.0 / 60.0) / F32(10.0)))
    return dict(particles=ps, params=params, colliders=[], cell_width=h, grid_capacity=100_000,
                model=MODEL_COROTATED)


def reference_sand3():
    """The reference's shipping 3D scene as written (crates/wgsparkl3d/examples/sand3.rs:28-113): 45 x 100 x 45 = 202 500
    Drucker-Prager sand particles (E = 2e9, nu = 0.2, phase None) at spacing h/2 above a floor cuboid, four wall cuboids
    and one kinematic cuboid (tilted -0.5 rad about z, spinning at -1 rad/s about y); h = 1, dt = 1/1200, capacity 60 000."""
    import math
    h, nxz = 1.0, 45
    i, j, k = np.meshgrid(np.arange(nxz), np.arange(100), np.arange(nxz), indexing="ij")
    pos = (np.stack([i.ravel() + 0.5 - nxz / 2.0, j.ravel() + 0.5 + 10.0, k.ravel() + 0.5 - nxz / 2.0], 1) * (h / 2.0)).astype(F32)
    ps = ParticleSet.uniform(pos, h / 4.0, 2700.0, ElasticCoefficients.from_young_modulus(2.0e9, 0.2),
                             plasticity=DruckerPrager.new(2.0e9, 0.2), phase=None)
    colliders = [Collider.cuboid((100.0, 4.0, 100.0), (0.0, -4.0, 0.0)),
                 Collider.cuboid((35.0, 5.0, 0.5), (0.0, 5.0, -35.0)), Collider.cuboid((35.0, 5.0, 0.5), (0.0, 5.0, 35.0)),
                 Collider.cuboid((0.5, 5.0, 35.0), (-35.0, 5.0, 0.0)), Collider.cuboid((0.5, 5.0, 35.0), (35.0, 5.0, 0.0)),
                 Collider.cuboid((0.5, 2.0, 30.0), (0.0, 2.0, 0.0), rotation=(0.0, 0.0, math.sin(-0.25), math.cos(-0.25)),
                                 angvel=(0.0, -1.0, 0.0))]
    return dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=(1.0 / 60.0) / 20.0), colliders=colliders,
                cell_width=h, grid_capacity=60_000, model=MODEL_COROTATED,
                name="the reference's sand3 example as shipped: 45x100x45 Drucker-Prager sand, floor + 4 walls + kinematic rotating cuboid",
                bytes_per_particle=216.0)


def reference_sand2():
    """The reference's largest shipping scene as written (crates/wgsparkl2d/examples/sand2.rs:21-175): 700 x 700 = 490 000
    Drucker-Prager sand particles (E = 1e7, nu = 0.2, rho = 1000, phase None) at spacing h/2 with h = 0.2, lifted by 46; a floor
    and two tilted walls (fixed cuboids), three spinning cuboids, a spinning ball and a spinning capsule (kinematic), eight
    dynamic cuboids of density 10 + 100 k dropped from y = 120; dt = 1/600, capacity 60 000. That is 16 coupled colliders,
    the reference's limit (quirk B11). rapier's body-body contacts are not part of the MPM path: the dynamic cuboids move
    under gravity and the sand's impulses."""
    h = 0.2
    i, j = np.meshgrid(np.arange(700), np.arange(700), indexing="ij")
    pos = (np.stack([i.ravel() + 0.5, j.ravel() + 0.5], 1) * (h / 2.0)).astype(F32)
    pos[:, 1] += F32(46.0)
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, ElasticCoefficients.from_young_modulus(1.0e7, 0.2),
                             plasticity=DruckerPrager.new(1.0e7, 0.2), phase=None)
    w = 1.0
    colliders = [Collider.cuboid((42.0, 1.0), (35.0, -1.0), rotation=(0.0,)),
                 Collider.cuboid((1.0, 52.0), (-25.0, 45.0), rotation=(0.5,)), Collider.cuboid((1.0, 52.0), (95.0, 45.0), rotation=(-0.5,)),
                 Collider.cuboid((1.0, 10.0), (5.0, 35.0), rotation=(0.0,), angvel=(w,)),
                 Collider.cuboid((10.0, 1.0), (35.0, 35.0), rotation=(0.0,), angvel=(-w,)),
                 Collider.cuboid((1.0, 10.0), (65.0, 35.0), rotation=(0.0,), angvel=(w,)),
                 Collider.ball(5.0, (20.0, 20.0), rotation=(0.0,), angvel=(-w,)),
                 Collider(SHAPE_CAPSULE, (5.0, 3.0), (50.0, 20.0), rotation=(0.0,), angvel=(-w,))]
    for k in range(8):
        colliders.append(Collider.cuboid((5.0, 1.0), (35.0 + 3.0 * k, 120.0), rotation=(0.0,)).with_density(10.0 + 100.0 * k, 2))
    return dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81), dt=(1.0 / 60.0) / 10.0), colliders=colliders,
                cell_width=h, grid_capacity=60_000, model=MODEL_COROTATED,
                name="the reference's sand2 example as shipped (2D): 700x700 Drucker-Prager sand, h = 0.2, 16 coupled colliders "
                     "(3 fixed, 5 kinematic spinning, 8 dynamic cuboids)",
                bytes_per_particle=144.0)


def elastic_block_2d(nx=100, ny=100, with_floor=True, jitter=0.05):
    """C1: wgsparkl2d elastic block, 10k particles, 64x64 grid (8x8 blocks), corotated."""
    h = 1.0
    pos = lattice((nx, ny), (7.0, 7.0), h, jitter)
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, ElasticCoefficients.from_young_modulus(5.0e6, 0.2),
                             phase=ParticlePhase(1.0, FLT_MAX))
    colliders = [Collider.cuboid((1000.0, 1.0), (0.0, 1.0), rotation=(0.0,))] if with_floor else []
    params = SimulationParams(gravity=(0.0, -9.81), dt=1.0 / 900.0)
    return dict(particles=ps, params=params, colliders=colliders, cell_width=h, grid_capacity=256,
                model=MODEL_COROTATED)


def neo_hookean_cube(n_side=100, with_floor=False, jitter=0.05, cell_width=1.0, grid_capacity=None):
    """C2: n_side^3 particles (n_side/2)^3 cells inside a 128^3-cell domain, neo-Hookean,
    E = 1e7, nu = 0.2, rho = 2700, phase = 1 (never fractures), dt = 1/1200."""
    h = cell_width
    origin = (20.0 * h, 8.0 * h, 20.0 * h)
    pos = lattice((n_side,) * 3, origin, h, jitter)
    ps = ParticleSet.uniform(pos, h / 4.0, 2700.0, ElasticCoefficients.from_young_modulus(1.0e7, 0.2),
                             phase=ParticlePhase(1.0, FLT_MAX))
    colliders = [Collider.cuboid((1000.0 * h, 2.0 * h, 1000.0 * h), (0.0, 0.0, 0.0))] if with_floor else []
    params = SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0 / 1200.0)
    if grid_capacity is None:
        nb = (n_side // 8 + 3) ** 3
        grid_capacity = max(1024, 1 << int(np.ceil(np.log2(nb * 1.5))))
    return dict(particles=ps, params=params, colliders=colliders, cell_width=h,
                grid_capacity=grid_capacity, model=MODEL_NEO_HOOKEAN)


def corotated_cube_with_paddle(n_side=200, jitter=0.05, cell_width=1.0, paddle_speed=0.8):
    """C4 (single-GPU form): n_side^3 corotated elastic particles on the floor cuboid, hit by one kinematic rotating
    cuboid (the `sand3.rs:95-103` pattern: a body whose angular velocity is set by the host and whose pose the
    device integrates every substep)."""
    sc = neo_hookean_cube(n_side=n_side, with_floor=True, jitter=jitter, cell_width=cell_width)
    h = cell_width
    sc["model"] = MODEL_COROTATED
    side = n_side * h / 2.0
    sc["particles"].pos[:, 1] -= 5.6 * h                       # resting on the floor (top face at y = 2 h)
    centre = (20.0 * h + side + 2.2 * h, 2.4 * h + side / 2.0, 20.0 * h + side / 2.0)
    sc["colliders"].append(Collider.cuboid((2.0 * h, side / 2.0, side / 3.0), centre, angvel=(0.0, paddle_speed, 0.0),
                                           linvel=(-2.0, 0.0, 0.0)))
    return sc


def sand_column(nx=100, ny=400, nz=100, with_floor=False, jitter=0.05, grid_capacity=None, with_walls=False):
    """C3: Drucker-Prager sand column (sand3.rs:45-46 material), corotated stress, phase None. `with_walls`: the floor
    and four walls of SURVEY 8d C3 (five cuboid colliders; the walls stand 1.5 cells off the column's faces)."""
    h = 1.0
    origin = (20.0, 8.0, 20.0)
    pos = lattice((nx, ny, nz), origin, h, jitter)
    ps = ParticleSet.uniform(pos, h / 4.0, 2700.0, ElasticCoefficients.from_young_modulus(2.0e9, 0.2),
                             plasticity=DruckerPrager.new(2.0e9, 0.2), phase=None)
    colliders = [Collider.cuboid((1000.0, 2.0, 1000.0), (0.0, 0.0, 0.0))] if (with_floor or with_walls) else []
    if with_walls:
        x0, x1 = origin[0] - 1.5 * h, origin[0] + nx * h / 2.0 + 1.5 * h
        z0, z1 = origin[2] - 1.5 * h, origin[2] + nz * h / 2.0 + 1.5 * h
        t = 2.0 * h                                                # wall half thickness
        colliders += [Collider.cuboid((t, 1000.0, 1000.0), (x0 - t, 0.0, 0.0)), Collider.cuboid((t, 1000.0, 1000.0), (x1 + t, 0.0, 0.0)),
                      Collider.cuboid((1000.0, 1000.0, t), (0.0, 0.0, z0 - t)), Collider.cuboid((1000.0, 1000.0, t), (0.0, 0.0, z1 + t))]
    params = SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0 / 1200.0)
    if grid_capacity is None:
        nb = (nx // 8 + 3) * (ny // 8 + 3) * (nz // 8 + 3)
        grid_capacity = max(1024, 1 << int(np.ceil(np.log2(nb * 1.5))))
    return dict(particles=ps, params=params, colliders=colliders, cell_width=h,
                grid_capacity=grid_capacity, model=MODEL_COROTATED)


def random_cloud(n, dim=3, extent=12.0, cell_width=1.0, seed=7, vel_scale=1.0,
                 young=1.0e5, nu=0.3, density=10.0, plasticity=None, phase=None,
                 perturb_F=0.05, perturb_C=0.5):
    """Unstructured test cloud with random velocities, F and APIC matrices
    (exercises every term of P2G / G2P; ragged cells, empty cells)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(1.5 * cell_width, extent * cell_width, size=(n, dim)).astype(F32)
    ps = ParticleSet.uniform(pos, cell_width / 4.0, density,
                             ElasticCoefficients.from_young_modulus(young, nu),
                             plasticity=plasticity, phase=phase)
    ps.vel[:] = rng.normal(0.0, vel_scale, size=(n, dim)).astype(F32)
    eye = np.eye(dim, dtype=F32).reshape(-1)
    ps.def_grad[:] = eye + rng.normal(0.0, perturb_F, size=(n, dim * dim)).astype(F32)
    ps.affine[:] = (rng.normal(0.0, perturb_C, size=(n, dim * dim)) * ps.mass[:, None]).astype(F32)
    ps.mass[:] = (ps.mass * rng.uniform(0.5, 1.5, size=n)).astype(F32)
    return ps


def _hash_jitter(ids: np.ndarray, dim: int, amplitude: float) -> np.ndarray:
    """Deterministic per-particle jitter from the GLOBAL particle id (so that every rank of a sharded run
    generates exactly the particles a single-domain run would): splitmix64 -> uniform in [-a, a)."""
    out = np.empty((len(ids), dim), np.float64)
    for k in range(dim):
        z = (ids.astype(np.uint64) * np.uint64(dim) + np.uint64(k) + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        out[:, k] = (z >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    return (out * 2.0 - 1.0) * amplitude


def neo_hookean_bar(n_side=100, world=1, rank=None, jitter=0.05, cell_width=1.0):
    """Weak-scaling workload: `world` C2 cubes side by side along x = one elastic bar of
    (n_side * world) x n_side x n_side particles. With `rank` given, only the particles of that rank's
    x-slab are generated (global ids = index in the full lattice); returns the slab partition too."""
    from .sharded import SlabPartition, associated_block_x
    h = cell_width
    ox, oy, oz = 20.0 * h, 8.0 * h, 20.0 * h
    nx = n_side * world
    # slab cuts in blocks (4 cells): the block containing the first lattice plane of each rank
    cuts = [int(np.floor((ox / h - 1.0) / 4.0))]
    for r in range(1, world):
        cuts.append(int(np.round((ox / h + n_side * r / 2.0 - 1.0) / 4.0)))
    cuts.append(int(np.floor((ox / h + nx / 2.0) / 4.0)) + 2)
    part = SlabPartition(cuts)
    if rank is None:
        i0, i1 = 0, nx
    else:
        i0, i1 = max(0, n_side * rank - 12), min(nx, n_side * (rank + 1) + 12)
    i, j, k = np.meshgrid(np.arange(i0, i1), np.arange(n_side), np.arange(n_side), indexing="ij")
    idx = np.stack([i.ravel(), j.ravel(), k.ravel()], 1)
    gid = ((idx[:, 0].astype(np.int64) * n_side + idx[:, 1]) * n_side + idx[:, 2])
    pos = (idx + 0.5) * (h / 2.0) + np.array([ox, oy, oz])
    if jitter:
        pos = pos + _hash_jitter(gid, 3, jitter * h)
    pos = pos.astype(F32)
    if rank is not None:
        own = part.owner_of_blocks(associated_block_x(pos, h, 3)) == rank
        pos, gid = pos[own], gid[own]
    ps = ParticleSet.uniform(pos, h / 4.0, 2700.0, ElasticCoefficients.from_young_modulus(1.0e7, 0.2),
                             phase=ParticlePhase(1.0, FLT_MAX))
    nb = (n_side // 8 + 4) ** 2 * (n_side // 8 + 8)
    return dict(particles=ps, global_ids=gid.astype(np.uint32), partition=part,
                params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0 / 1200.0),
                colliders=[Collider.cuboid((100000.0 * h, 2.0 * h, 1000.0 * h), (0.0, 0.0, 0.0))],
                cell_width=h, grid_capacity=max(1024, 1 << int(np.ceil(np.log2(nb * 1.5)))), model=MODEL_NEO_HOOKEAN,
                global_particles=nx * n_side * n_side)


def _slab_block(counts, origin, h, jitter, world, rank, cuts=None):
    """Lattice block of counts[0] x counts[1] x counts[2] particles (spacing h/2, hashed jitter by GLOBAL id) cut into
    `world` x-slabs of (nearly) equal particle count, cuts on block boundaries. With `rank` given only that slab is
    generated. Returns (pos, global ids, SlabPartition)."""
    from .sharded import SlabPartition, associated_block_x
    nx, ny, nz = counts
    ox = origin[0]
    if cuts is None:
        # the block column of lattice plane i is floor((round((ox + (i + .5) h/2) / h) - 1) / 4); cut r sits at the
        # block boundary closest to the plane that splits the particle count evenly
        cuts = [int(np.floor((ox / h - 1.0) / 4.0))]
        for r in range(1, world):
            cuts.append(int(np.round((ox / h + (nx * r / world) / 2.0 - 1.0) / 4.0)))
        cuts.append(int(np.floor((ox / h + nx / 2.0) / 4.0)) + 2)
        for i in range(1, len(cuts)):
            cuts[i] = max(cuts[i], cuts[i - 1] + 1)
    part = SlabPartition(cuts)
    if rank is None:
        i0, i1 = 0, nx
    else:
        # lattice planes that can fall into this rank's block range (+ a margin for the jitter)
        lo_b, hi_b = part.cuts[rank], part.cuts[rank + 1]
        i0 = 0 if rank == 0 else max(0, int(np.floor(((lo_b * 4 + 0.5) * h - ox) * 2.0 / h)) - 3)
        i1 = nx if rank == world - 1 else min(nx, int(np.ceil(((hi_b * 4 + 1.5) * h - ox) * 2.0 / h)) + 3)
    i, j, k = np.meshgrid(np.arange(i0, i1, dtype=np.int32), np.arange(ny, dtype=np.int32), np.arange(nz, dtype=np.int32), indexing="ij")
    gid = (i.ravel().astype(np.int64) * ny + j.ravel()) * nz + k.ravel()
    pos = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64)
    del i, j, k
    pos = (pos + 0.5) * (h / 2.0) + np.asarray(origin, np.float64)
    if jitter:
        pos += _hash_jitter(gid, 3, jitter * h)
    pos = pos.astype(F32)
    if rank is not None:
        own = part.owner_of_blocks(associated_block_x(pos, h, 3)) == rank
        pos, gid = pos[own], gid[own]
    return pos, gid.astype(np.uint32), part


def fluid_block(nx=256, ny=250, nz=250, world=1, rank=None, jitter=0.05, cell_width=1.0, with_floor=True,
                density=1000.0, bulk_modulus=1.0e7, grid_capacity=None):
    """C5 (BASELINE.json configs[4]): weakly-compressible "fluid" = pressure-only neo-Hookean
    (mu = 0 in src/models/neo_hookean_elasticity.wgsl:14-25 => tau = lambda * ln(J) * I; the reference has no fluid
    model of its own), nx x ny x nz = 16 M particles at 8 per cell inside a 512^3-cell domain, over the floor cuboid.
    lambda = bulk modulus 1e7 (sound speed 100 cells/s against h/dt = 1200), rho = 1000, dt = 1/1200, phase = 1.
    `world` / `rank`: the x-slab of one rank of a strong-scaling run (global ids = index in the full lattice, jitter
    hashed from the id, so every decomposition generates the very same particles)."""
    h = cell_width
    # x origin 16.5 h: lattice planes 2i, 2i + 1 sit at (16.75 + i) h and (17.25 + i) h, both inside cell 16 + i, so
    # 8 planes fill a block column exactly and equal block ranges are equal particle counts
    origin = (16.5 * h, 8.0 * h, 20.0 * h)
    pos, gid, part = _slab_block((nx, ny, nz), origin, h, jitter, world, rank)
    ps = ParticleSet.uniform(pos, h / 4.0, density, ElasticCoefficients(bulk_modulus, 0.0),
                             phase=ParticlePhase(1.0, FLT_MAX))
    colliders = [Collider.cuboid((100000.0 * h, 2.0 * h, 100000.0 * h), (0.0, 0.0, 0.0))] if with_floor else []
    if grid_capacity is None:
        slab_nx = nx if rank is None else -(-nx // world) + 16
        nb = (slab_nx // 8 + 4) * (ny // 8 + 4) * (nz // 8 + 4)
        grid_capacity = max(1024, 1 << int(np.ceil(np.log2(nb * 1.5))))
    return dict(particles=ps, global_ids=gid, partition=part,
                params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0 / 1200.0), colliders=colliders,
                cell_width=h, grid_capacity=grid_capacity, model=MODEL_NEO_HOOKEAN, global_particles=nx * ny * nz)


def tait_fluid_block(nx=256, ny=250, nz=250, world=1, rank=None, jitter=0.05, cell_width=1.0, with_floor=True,
                     density=1000.0, bulk_modulus=1.0e7, viscosity=0.0, gamma=7.0, grid_capacity=None):
    """The lattice of `fluid_block` under MODEL_FLUID: Tait pressure with bulk modulus `bulk_modulus` and exponent `gamma`
    (scene key "fluid_gamma", see the key table of this module), dynamic viscosity `viscosity`. Same particles, ids and slabs as
    `fluid_block` for the same arguments; to first order in J - 1 the same pressure."""
    sc = fluid_block(nx, ny, nz, world=world, rank=rank, jitter=jitter, cell_width=cell_width, with_floor=with_floor,
                     density=density, bulk_modulus=bulk_modulus, grid_capacity=grid_capacity)
    ps = sc["particles"]
    ps.lambda_[:], ps.mu[:] = FluidCoefficients(bulk_modulus, viscosity).arrays(ps.n)
    sc["model"] = MODEL_FLUID
    sc["fluid_gamma"] = float(gamma)
    return sc


def _container(walls):
    if walls not in ("colliders", "grid"):
        raise ValueError(f"walls={walls!r}: 'colliders' (CPIC cuboids) or 'grid' (domain walls, scene key \"walls\")")
    return walls == "grid"


def dam_break(nx=24, ny=40, nz=16, jitter=0.05, cell_width=1.0, density=1000.0, bulk_modulus=2.0e5, viscosity=0.0, gamma=7.0,
              walls="colliders", wall_type=WALL_SLIP, wall_friction=0.0):
    """Small dam break for tests: a column of Tait fluid (MODEL_FLUID) standing on the floor cuboid, one face against a wall
    cuboid, free to collapse along +x. Both colliders are within reach of the column from the first substep, so the
    near-collider list walk and the CPIC paths of the fused G2P advance fluid particles at once.
    `walls="grid"`: no cuboids; the same floor and wall as domain walls (scene key "walls"), their planes on the cuboids' faces."""
    h = cell_width
    origin = (8.3 * h, 2.2 * h, 8.0 * h)                       # floor top at y = 2 h, wall face at x = 8 h
    pos = lattice((nx, ny, nz), origin, h, jitter)
    ps = ParticleSet.uniform(pos, h / 4.0, density, FluidCoefficients(bulk_modulus, viscosity), phase=ParticlePhase(1.0, FLT_MAX))
    colliders = [Collider.cuboid((1000.0 * h, 2.0 * h, 1000.0 * h), (0.0, 0.0, 0.0)),
                 Collider.cuboid((2.0 * h, 1000.0 * h, 1000.0 * h), (6.0 * h, 0.0, 0.0))]
    sc = dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0 / 1200.0), colliders=colliders,
              cell_width=h, grid_capacity=4096, model=MODEL_FLUID, fluid_gamma=float(gamma))
    if _container(walls):
        sc["colliders"] = []
        sc["walls"] = [Wall.low(8.0 * h, h, wall_type, wall_friction), None, Wall.low(2.0 * h, h, wall_type, wall_friction), None, None, None]
    return sc


def block_in_fluid(dim=3, tank=(24, 16, 16), block=8, gap=0.5, drop_speed=0.0, solid_model=MODEL_NEO_HOOKEAN, jitter=0.05, cell_width=1.0,
                   density=1000.0, bulk_modulus=2.0e5, viscosity=0.0, gamma=7.0, solid_density=2000.0, young_modulus=2.0e5, poisson=0.3,
                   walls="colliders", wall_type=WALL_SLIP, wall_friction=0.0):
    """Fluid and solid in one simulation (scene key "models", see the key table of this module): a tank of Tait fluid — `tank` particles at spacing h/2 standing on
    the floor cuboid between four wall cuboids (two in 2D), like `dam_break` but closed — and an elastic block of `block`^dim particles
    hanging `gap` cells above the middle of its surface, falling at `drop_speed`. The two interact through the grid alone. Returns the
    scene dict with "models" (np.uint8 per particle: MODEL_FLUID for the tank, `solid_model` for the block) and "solid_model";
    "model" (the data's single model, before the table is set) is the solid's: selecting the fluid for the whole data would collapse the
    block's deformation gradient too. The fluid's particles come first.
    `walls="grid"`: no cuboids; the same tank as domain walls (scene key "walls": the floor and the side faces, open at the top), their
    planes on the first node at or beyond the cuboids' faces."""
    h = cell_width
    tank = tuple(tank)[:dim] if dim == 3 else (tank[0], tank[1])
    origin = (8.3 * h, 2.2 * h, 8.3 * h)[:dim]                 # floor top at y = 2 h, wall faces 0.3 h off the fluid
    fpos = lattice(tank, origin, h, jitter)
    top = origin[1] + tank[1] * h / 2.0
    borigin = [origin[k] + (tank[k] - block) * h / 4.0 for k in range(dim)]
    borigin[1] = top + gap * h
    bpos = lattice((block,) * dim, borigin, h, jitter, seed=4321)
    fluid = FluidCoefficients(bulk_modulus, viscosity)
    ps = ParticleSet.uniform(np.concatenate([fpos, bpos]), h / 4.0, density, fluid, phase=ParticlePhase(1.0, FLT_MAX))
    nf = len(fpos)
    solid = ElasticCoefficients.from_young_modulus(young_modulus, poisson)
    ps.lambda_[nf:], ps.mu[nf:] = F32(solid.lambda_), F32(solid.mu)
    ps.mass[nf:] = (ps.init_volume[nf:] * F32(solid_density)).astype(F32)
    ps.vel[nf:, 1] = F32(-drop_speed)
    t, big = 2.0 * h, 1000.0 * h
    x0, x1 = origin[0] - 0.3 * h, origin[0] + tank[0] * h / 2.0 + 0.3 * h
    if dim == 3:
        z0, z1 = origin[2] - 0.3 * h, origin[2] + tank[2] * h / 2.0 + 0.3 * h
        colliders = [Collider.cuboid((big, t, big), (0.0, 0.0, 0.0)),
                     Collider.cuboid((t, big, big), (x0 - t, 0.0, 0.0)), Collider.cuboid((t, big, big), (x1 + t, 0.0, 0.0)),
                     Collider.cuboid((big, big, t), (0.0, 0.0, z0 - t)), Collider.cuboid((big, big, t), (0.0, 0.0, z1 + t))]
    else:
        colliders = [Collider.cuboid((big, t), (0.0, 0.0), rotation=(0.0,)),
                     Collider.cuboid((t, big), (x0 - t, 0.0), rotation=(0.0,)), Collider.cuboid((t, big), (x1 + t, 0.0), rotation=(0.0,))]
    models = np.full(ps.n, MODEL_FLUID, np.uint8)
    models[nf:] = solid_model
    sc = dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0), colliders=colliders,
              cell_width=h, grid_capacity=4096, model=int(solid_model), fluid_gamma=float(gamma), models=models, solid_model=int(solid_model))
    if _container(walls):
        sc["colliders"] = []
        sc["walls"] = [Wall.low(x0, h, wall_type, wall_friction), Wall.high(x1, h, wall_type, wall_friction),
                       Wall.low(2.0 * h, h, wall_type, wall_friction), None]
        if dim == 3:
            sc["walls"] += [Wall.low(z0, h, wall_type, wall_friction), Wall.high(z1, h, wall_type, wall_friction)]
    return sc


def walled_box(dim=3, n=6000, lo=2, hi=18, wall_type=WALL_SLIP, friction=0.0, cell_width=1.0, speed=1.0, seed=11, with_walls=True,
               young=2.0e4, density=10.0):
    """A cloud thrown at all 2 * dim faces of a box of domain walls, no colliders, no gravity: `n` soft elastic particles scattered
    over the cells (lo + 2 .. hi - 2)^dim, each moving away from the centre of the box at up to `speed` times the grid's cap h / dt. The low planes are `lo`, the high planes `hi` (scene key "walls"; `with_walls=False`: none, the cloud flies apart)."""
    h = float(cell_width)
    rng = np.random.default_rng(seed)
    pos = rng.uniform((lo + 2.0) * h, (hi - 2.0) * h, size=(n, dim)).astype(F32)
    ps = ParticleSet.uniform(pos, h / 4.0, density, ElasticCoefficients.from_young_modulus(young, 0.3), phase=ParticlePhase(1.0, FLT_MAX))
    params = SimulationParams(gravity=(0.0,) * dim, dt=1.0 / 1200.0)
    # (away from the centre: neighbours move alike, so the transfers do not average the motion away as they would random directions)
    direction = pos.astype(np.float64) - 0.5 * (lo + hi) * h + rng.normal(0.0, 0.05 * h, size=(n, dim))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    ps.vel[:] = (direction * rng.uniform(0.5, 1.0, size=(n, 1)) * (speed * h / params.dt)).astype(F32)
    walls = [Wall(int(wall_type), float(friction), int(lo if f % 2 == 0 else hi)) for f in range(2 * dim)] if with_walls else None
    return dict(particles=ps, params=params, colliders=[], cell_width=h, grid_capacity=4096, model=MODEL_COROTATED, walls=walls)


def snowball(dim=3, radius=6.0, cell_width=1.0, speed=0.01, gap=0.5, snow=None, young_modulus=1.4e5, poisson=0.2, density=400.0,
             jitter=0.05, plasticity=PLASTICITY_SNOW):
    """A ball of snow thrown at a sticky domain wall (scene keys "plasticity" and "walls"): particles at spacing h/2 inside a ball of
    `radius` cells, moving along -x at `speed` times the grid's cap h / dt (the default: 10 m/s, half the material's speed of sound) towards the sticky
    low x face `gap` cells in front of it;
    no colliders, gravity along -y. The material is that of Stomakhin et al. 2013 (E = 1.4e5, nu = 0.2, rho = 400) under
    `models.Snow()` (or `snow`): the ball flattens against the wall, hardens where it is compressed and breaks up where it is
    stretched. `plasticity=PLASTICITY_DRUCKER_PRAGER` gives the same particles as Drucker-Prager sand of the same stiffness (the
    timing twin of notes/round_31.md)."""
    h = float(cell_width)
    n_side = int(np.ceil(4.0 * radius)) + 1
    origin = tuple([4.0 * h + gap * h] + [4.0 * h] * (dim - 1))
    pos = lattice((n_side,) * dim, origin, h, jitter)
    centre = np.asarray(origin, np.float64) + 0.25 * n_side * h
    pos = pos[np.linalg.norm(pos.astype(np.float64) - centre, axis=1) <= radius * h]
    rule = (snow or Snow()) if plasticity == PLASTICITY_SNOW else DruckerPrager.new(young_modulus, poisson)
    ps = ParticleSet.uniform(pos, h / 4.0, density, ElasticCoefficients.from_young_modulus(young_modulus, poisson), plasticity=rule, phase=None)
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0e-3)
    ps.vel[:, 0] = F32(-speed * h / params.dt)
    walls = [Wall.low(4.0 * h, h, WALL_STICKY), None] + [None] * (2 * dim - 2)
    return dict(particles=ps, params=params, colliders=[], cell_width=h, grid_capacity=4096, model=MODEL_COROTATED,
                plasticity=int(plasticity), walls=walls,
                name=f"snowball {dim}D: {ps.n} particles, radius {radius} cells, thrown at a sticky wall at {speed} h/dt")


def planetoid(dim=3, radius=5.0, cell_width=1.0, speed=0.05, attraction=None, jitter=0.05, young_modulus=10.0, density=10.0, with_field=True):
    """A ball thrown apart and held together by a central attraction (scene key "forces"): particles at spacing h/2 inside a ball of
    `radius` cells, each moving away from the centre at `speed` times the grid's cap h / dt times its distance over the radius; no
    gravity, no colliders, no walls; one RADIAL field of falloff 0 at the centre — a spring of `attraction` per second squared.
    With alpha = speed h / dt / (radius h) the outward rate, a particle under the spring alone reaches sqrt(1 + alpha^2 / attraction)
    times its start distance: the default, (0.8 alpha)^2, turns every particle round at 1.6 times its own, inside twice the start
    radius. The material is next to pressureless (the corotated energy grows with the sixth power of a dilation: anything stiffer
    holds the ball together by itself), so nothing but the field does. `with_field=False`: the control, which flies apart."""
    h = float(cell_width)
    n_side = int(np.ceil(4.0 * radius)) + 1
    origin = (6.0 * h,) * dim
    pos = lattice((n_side,) * dim, origin, h, jitter)
    centre = np.asarray(origin, np.float64) + 0.25 * n_side * h
    rel = pos.astype(np.float64) - centre
    keep = np.linalg.norm(rel, axis=1) <= radius * h
    pos, rel = pos[keep], rel[keep]
    ps = ParticleSet.uniform(pos, h / 4.0, density, ElasticCoefficients.from_young_modulus(young_modulus, 0.3), phase=ParticlePhase(1.0, FLT_MAX))
    params = SimulationParams(gravity=(0.0,) * dim, dt=1.0e-3)
    v_out = speed * h / params.dt
    ps.vel[:] = (rel * (v_out / (radius * h))).astype(F32)
    k = float(attraction) if attraction is not None else (0.8 * v_out / (radius * h)) ** 2
    forces = [ForceField.radial(tuple(float(c) for c in centre), k)] if with_field else None
    return dict(particles=ps, params=params, colliders=[], cell_width=h, grid_capacity=8192, model=MODEL_COROTATED, forces=forces,
                centre=centre, start_radius=radius * h,
                name=f"planetoid {dim}D: {ps.n} particles thrown apart at {speed} h/dt, held by a central spring of {k:.3g} / s^2")


def vortex_tank(dim=3, tank=(24, 12, 24), cell_width=1.0, spin=40.0, drag_rate=20.0, jitter=0.05, density=1000.0, bulk_modulus=2.0e5,
                viscosity=0.0, gamma=7.0):
    """A stirred tank (scene keys "walls" and "forces"): Tait fluid (MODEL_FLUID), `tank` particles at spacing h/2, between slip domain
    walls (floor and side faces, open at the top) under gravity; a VORTEX of falloff 0 about the vertical line through the middle of the
    tank (2D: about +z through its middle) spins it up at `spin` per second squared, and a DRAG zone — a box over the lowest two cells
    of the tank, its faces half-way between nodes — damps the flow along the floor at `drag_rate` per second."""
    h = float(cell_width)
    tank = tuple(tank)[:dim] if dim == 3 else (tank[0], tank[1])
    origin = (8.3 * h, 2.2 * h, 8.3 * h)[:dim]
    ps = ParticleSet.uniform(lattice(tank, origin, h, jitter), h / 4.0, density, FluidCoefficients(bulk_modulus, viscosity),
                             phase=ParticlePhase(1.0, FLT_MAX))
    lo = [origin[k] - 0.3 * h for k in range(dim)]
    hi = [origin[k] + tank[k] * h / 2.0 + 0.3 * h for k in range(dim)]
    walls = [Wall.low(lo[0], h), Wall.high(hi[0], h), Wall.low(2.0 * h, h), None]
    if dim == 3:
        walls += [Wall.low(lo[2], h), Wall.high(hi[2], h)]
    mid = [0.5 * (lo[k] + hi[k]) for k in range(dim)]
    floor_zone_centre = list(mid)
    floor_zone_centre[1] = 3.0 * h
    half = [1000.0 * h] * dim
    half[1] = 1.5 * h                                            # nodes 2, 3 and 4 along y: faces at 1.5 h and 4.5 h
    forces = [ForceField.vortex(mid, spin, axis=(0.0, 1.0, 0.0)), ForceField.drag(drag_rate).within_box(floor_zone_centre, half)]
    return dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0), colliders=[], cell_width=h,
                grid_capacity=4096, model=MODEL_FLUID, fluid_gamma=float(gamma), walls=walls, forces=forces,
                name=f"vortex tank {dim}D: {ps.n} fluid particles between grid walls, stirred by a vortex, damped along the floor")


def _nozzle(dim, proto, centre, across, rows, h, dt, speed, batches, jitter, seed, **kw):
    """an emitter pouring along -y: a lattice of `across` points per horizontal axis and `rows` layers at spacing h/2, centred on
    `centre` (its low corner kept on the h/4 lattice), its prototype falling at `speed` times h / dt, one slab per period"""
    count = tuple(rows if k == 1 else across for k in range(dim))
    lo = tuple(float(np.floor((centre[k] - count[k] * h / 4.0) / (h / 4.0)) * (h / 4.0)) for k in range(dim))
    proto.vel[0, 1] = F32(-speed * h / dt)
    return Emitter.nozzle(proto, lo, count, h / 2.0, dt, jitter=jitter, seed=seed, batches=batches, **kw)


def faucet(dim=3, tank=8, across=4, rows=1, height=10.0, speed=0.0625, batches=32, cell_width=1.0, jitter=0.1, density=1000.0,
           bulk_modulus=2.0e5, viscosity=0.0, gamma=7.0, seed=2024):
    """A faucet filling a tank (scene keys "particle_capacity" and "emitters"): the data starts EMPTY; one emitter `height` cells above
    the floor pours Tait fluid (MODEL_FLUID) — `across`^(dim-1) x `rows` particles per batch at spacing h/2, falling at `speed` times the
    grid's cap h / dt, a new slab whenever the last one has cleared the nozzle (`Emitter.nozzle`) — into a tank of slip domain walls
    `tank` cells wide (floor and side faces, open at the top). Room for `batches` batches, which is also the emitter's limit."""
    h = float(cell_width)
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0)
    fluid = FluidCoefficients(bulk_modulus, viscosity)
    empty = ParticleSet.uniform(np.zeros((0, dim), F32), h / 4.0, density, fluid, phase=ParticlePhase(1.0, FLT_MAX))
    proto = ParticleSet.uniform(np.zeros((1, dim), F32), h / 4.0, density, fluid, phase=ParticlePhase(1.0, FLT_MAX))
    lo_plane, hi_plane, floor = 4, 4 + int(tank), 2
    centre = [0.5 * (lo_plane + hi_plane) * h] * dim
    centre[1] = (floor + height) * h
    em = _nozzle(dim, proto, centre, across, rows, h, params.dt, speed, batches, jitter, seed)
    walls = [Wall(WALL_SLIP, 0.0, lo_plane), Wall(WALL_SLIP, 0.0, hi_plane), Wall(WALL_SLIP, 0.0, floor), None]
    if dim == 3:
        walls += [Wall(WALL_SLIP, 0.0, lo_plane), Wall(WALL_SLIP, 0.0, hi_plane)]
    return dict(particles=empty, params=params, colliders=[], cell_width=h, grid_capacity=4096, model=MODEL_FLUID, fluid_gamma=float(gamma),
                walls=walls, particle_capacity=int(batches) * em.batch_size, emitters=[em],
                name=f"faucet {dim}D: {em.batch_size} fluid particles every {em.period} substeps into a tank of grid walls, starting empty")


def sand_pour(dim=3, heap=(8, 2, 8), across=3, rows=1, height=8.0, speed=0.0625, batches=32, cell_width=1.0, jitter=0.1, density=2700.0,
              young_modulus=1.0e7, poisson=0.2, seed=2025):
    """Sand running onto a heap (scene keys "particle_capacity" and "emitters"): Drucker-Prager sand, a small starting heap of `heap`
    particles at spacing h/2 on the floor cuboid — so that the data's step carries plastic state from its creation on — and one emitter
    `height` cells above the floor pouring the same sand (bit for bit the heap's material: the uniform layouts hold it) onto it."""
    h = float(cell_width)
    heap = tuple(heap)[:dim] if dim == 3 else (heap[0], heap[1])
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0)
    sand = dict(model=ElasticCoefficients.from_young_modulus(young_modulus, poisson), plasticity=DruckerPrager.new(young_modulus, poisson), phase=None)
    origin = (8.0 * h, 2.2 * h, 8.0 * h)[:dim]                  # floor top at y = 2 h
    ps = ParticleSet.uniform(lattice(heap, origin, h, 0.05), h / 4.0, density, **sand)
    proto = ParticleSet.uniform(np.zeros((1, dim), F32), h / 4.0, density, **sand)
    centre = [origin[k] + heap[k] * h / 4.0 for k in range(dim)]
    centre[1] = (2.0 + height) * h
    em = _nozzle(dim, proto, centre, across, rows, h, params.dt, speed, batches, jitter, seed)
    floor = Collider.cuboid((1000.0 * h, 2.0 * h, 1000.0 * h), (0.0, 0.0, 0.0)) if dim == 3 else Collider.cuboid((1000.0 * h, 2.0 * h), (0.0, 0.0), rotation=(0.0,))
    return dict(particles=ps, params=params, colliders=[floor], cell_width=h, grid_capacity=4096, model=MODEL_COROTATED,
                particle_capacity=ps.n + int(batches) * em.batch_size, emitters=[em],
                name=f"sand pour {dim}D: {em.batch_size} sand particles every {em.period} substeps onto a heap of {ps.n} on a floor collider")


def ballistic_transit(position, velocity, gravity, dt, left, limit=100000):
    """Substeps a free particle (v += g dt, x += v dt: what an isolated MPM particle does) takes from `position` until `left(x)` is
    true — the scenes below size their particle capacity by it, and their tests the number of substeps to run."""
    x, v, g = np.asarray(position, np.float64).copy(), np.asarray(velocity, np.float64).copy(), np.asarray(gravity, np.float64)
    for k in range(1, limit + 1):
        v += g * dt
        x += v * dt
        if left(x):
            return k
    raise ValueError("ballistic_transit: the particle never leaves")


def _steady_capacity(em, transit, sink_period):
    """twice the particles in flight at a steady state: a batch every em.period substeps, each alive for `transit` substeps and up to
    one sink period more"""
    return 2 * (-(-(transit + sink_period) // em.period) + 1) * em.batch_size


def drain(dim=3, tank=8, across=4, rows=1, height=6.0, speed=0.0625, sink_period=4, cell_width=1.0, jitter=0.1, density=1000.0,
          bulk_modulus=2.0e5, viscosity=0.0, gamma=7.0, seed=2026):
    """A faucet over a drain (scene keys "emitters" and "sinks"): `faucet`'s emitter and walled tank, without a limit of batches, and a
    box sink over the two cell layers above and below the tank's floor, evaluated every `sink_period` substeps — what falls in is
    removed, so the run goes on at a bounded particle count. The capacity is twice the particles in flight at the steady state of a
    free fall (`ballistic_transit`; "transit_substeps" is that fall's length, for the caller)."""
    sc = faucet(dim, tank, across, rows, height, speed, 0, cell_width, jitter, density, bulk_modulus, viscosity, gamma, seed)
    h, em, params = float(cell_width), sc["emitters"][0], sc["params"]
    floor, mid = 2, (4 + 0.5 * tank) * h
    sink_top = (floor + 2) * h
    top = [em.lo[k] + em.count[k] * em.spacing for k in range(dim)]                      # the lattice's far corner, jitter included
    transit = ballistic_transit(top, em.proto.vel[0], params.gravity, params.dt, lambda x: x[1] <= sink_top - 0.25 * h)
    centre = [mid] * dim
    centre[1] = floor * h
    half = [(0.5 * tank + 2.0) * h] * dim
    half[1] = 2.0 * h
    sink = Sink.box(centre, half, period=int(sink_period))
    sc.update(particle_capacity=_steady_capacity(em, transit, int(sink_period)), sinks=[sink], transit_substeps=transit,
              name=f"drain {dim}D: {em.batch_size} fluid particles every {em.period} substeps into a walled tank, a sink over its floor every {sink_period}")
    return sc


def channel(dim=3, length=6.0, across=4, rows=1, speed=0.0625, sink_period=4, cell_width=1.0, jitter=0.1, density=1000.0,
            bulk_modulus=2.0e5, viscosity=0.0, gamma=7.0, seed=2027):
    """An open channel (scene keys "emitters" and "sinks"): the data starts EMPTY; an emitter on the low-x side throws Tait fluid along
    +x at `speed` times h / dt, and an OUTSIDE-box sink — the region of interest, `length` cells long behind the nozzle, 8 cells
    high and wide — removes everything that has left it, through its far face or, falling, through its bottom: inflow and outflow at
    a bounded particle count. Capacity and "transit_substeps" as in `drain`."""
    h = float(cell_width)
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0)
    fluid = FluidCoefficients(bulk_modulus, viscosity)
    empty = ParticleSet.uniform(np.zeros((0, dim), F32), h / 4.0, density, fluid, phase=ParticlePhase(1.0, FLT_MAX))
    proto = ParticleSet.uniform(np.zeros((1, dim), F32), h / 4.0, density, fluid, phase=ParticlePhase(1.0, FLT_MAX))
    proto.vel[0, 0] = F32(speed * h / params.dt)
    count = tuple(rows if k == 0 else across for k in range(dim))
    lo = (8.0 * h,) + (12.0 * h - across * h / 4.0,) * (dim - 1)
    em = Emitter.nozzle(proto, lo, count, h / 2.0, params.dt, jitter=jitter, seed=seed)
    centre = [8.0 * h + 0.5 * length * h] + [12.0 * h] * (dim - 1)
    half = [0.5 * length * h + h] + [4.0 * h] * (dim - 1)                                 # one cell of room behind the nozzle
    far, bottom = centre[0] + half[0], centre[1] - half[1]
    start = [lo[0] - 0.5 * h] + [lo[k] for k in range(1, dim)]                            # the slowest to leave: the nozzle's back, jitter included
    transit = ballistic_transit(start, proto.vel[0], params.gravity, params.dt, lambda x: x[0] > far + 0.25 * h or x[1] < bottom - 0.25 * h)
    sink = Sink.outside_box(centre, half, period=int(sink_period))
    return dict(particles=empty, params=params, colliders=[], cell_width=h, grid_capacity=4096, model=MODEL_FLUID, fluid_gamma=float(gamma),
                particle_capacity=_steady_capacity(em, transit, int(sink_period)), emitters=[em], sinks=[sink], transit_substeps=transit,
                name=f"channel {dim}D: {em.batch_size} fluid particles every {em.period} substeps along +x, an outflow box {length:g} cells long")


def config_scene(config="c2", world=1, rank=None, scaling="weak", n_side=None, jitter=0.05):
    """The BASELINE.json configs as (possibly sharded) scenes for bench.py: `c2` neo-Hookean cube (1 M), `c3`
    Drucker-Prager sand column standing between the floor and four walls (4 M), `c4` corotated cube + kinematic rotating
    cuboid (8 M), `c5` pressure-only neo-Hookean fluid block (16 M). world > 1: "strong" cuts the named size into `world` x-slabs, "weak" puts `world` copies side by
    side along x (fixed work per GPU). With `rank` given only that rank's slab is generated. Particles are identified
    by their index in the global lattice and jittered by a hash of it, so every decomposition simulates the same scene."""
    h = 1.0
    mult = world if scaling == "weak" else 1
    if config == "c5":
        nx, ny, nz = (256, 250, 250) if n_side is None else (n_side, n_side, n_side)
        sc = fluid_block(nx * mult, ny, nz, world=world, rank=rank, jitter=jitter)
        sc["name"] = f"wgsparkl3d weakly-compressible fluid (pressure-only neo-Hookean, mu = 0), {nx * mult}x{ny}x{nz} particles, 512^3-cell domain, floor cuboid"
        sc["bytes_per_particle"] = 160.0
        return sc
    if config == "c2":
        n = 100 if n_side is None else n_side
        counts, origin = (n * mult, n, n), (20.0 * h, 8.0 * h, 20.0 * h)
        model, elastic = MODEL_NEO_HOOKEAN, ElasticCoefficients.from_young_modulus(1.0e7, 0.2)
        plast, phase = None, ParticlePhase(1.0, FLT_MAX)
        colliders = [Collider.cuboid((100000.0 * h, 2.0 * h, 1000.0 * h), (0.0, 0.0, 0.0))]
        name = f"wgsparkl3d neo-Hookean elastic cube, {n * mult}x{n}x{n} particles, 128^3-cell domain, floor cuboid"
        bpp = 160.0
    elif config == "c3":
        nx, ny, nz = (100, 400, 100) if n_side is None else (n_side, 4 * n_side, n_side)
        counts, origin = (nx * mult, ny, nz), (20.0 * h, 2.2 * h, 20.0 * h)      # standing on the floor (top face y = 2)
        model, elastic = MODEL_COROTATED, ElasticCoefficients.from_young_modulus(2.0e9, 0.2)
        plast, phase = DruckerPrager.new(2.0e9, 0.2), None
        x0, x1 = origin[0] - 1.5 * h, origin[0] + counts[0] * h / 2.0 + 1.5 * h
        z0, z1 = origin[2] - 1.5 * h, origin[2] + nz * h / 2.0 + 1.5 * h
        t = 2.0 * h
        colliders = [Collider.cuboid((100000.0, 2.0, 1000.0), (0.0, 0.0, 0.0)),
                     Collider.cuboid((t, 1000.0, 1000.0), (x0 - t, 0.0, 0.0)), Collider.cuboid((t, 1000.0, 1000.0), (x1 + t, 0.0, 0.0)),
                     Collider.cuboid((100000.0, 1000.0, t), (0.0, 0.0, z0 - t)), Collider.cuboid((100000.0, 1000.0, t), (0.0, 0.0, z1 + t))]
        name = f"wgsparkl3d Drucker-Prager sand column, {nx * mult}x{ny}x{nz} particles, 256^3-cell domain, standing between the floor and four walls"
        bpp = 216.0
    elif config == "c4":
        # BASELINE.json configs[3]: corotated elastic cube resting on the floor, hit by one kinematic rotating cuboid — a body
        # whose velocity the host sets and whose pose the device integrates every substep (the pattern of
        # crates/wgsparkl3d/examples/sand3.rs:95-103); same geometry as corotated_cube_with_paddle, by global lattice
        # index so that it can be cut into x-slabs (every rank holds every collider).
        n = 200 if n_side is None else n_side
        counts, origin = (n * mult, n, n), (20.0 * h, 2.4 * h, 20.0 * h)
        model, elastic = MODEL_COROTATED, ElasticCoefficients.from_young_modulus(1.0e7, 0.2)
        plast, phase = None, ParticlePhase(1.0, FLT_MAX)
        sx, side = counts[0] * h / 2.0, n * h / 2.0
        colliders = [Collider.cuboid((100000.0 * h, 2.0 * h, 1000.0 * h), (0.0, 0.0, 0.0)),
                     Collider.cuboid((2.0 * h, side / 2.0, side / 3.0), (origin[0] + sx + 2.2 * h, origin[1] + side / 2.0, origin[2] + side / 2.0),
                                     angvel=(0.0, 0.8, 0.0), linvel=(-2.0, 0.0, 0.0))]
        name = (f"wgsparkl3d corotated elastic cube on the floor + kinematic rotating cuboid (rigid-body collision), {n * mult}x{n}x{n} particles, "
                "256^3-cell domain")
        bpp = 160.0
    else:
        raise ValueError(f"unknown config {config!r}")
    pos, gid, part = _slab_block(counts, origin, h, jitter, world, rank)
    ps = ParticleSet.uniform(pos, h / 4.0, 2700.0, elastic, plasticity=plast, phase=phase)
    slab_nx = counts[0] if rank is None else -(-counts[0] // world) + 16
    nb = (slab_nx // 8 + 4) * (counts[1] // 8 + 4) * (counts[2] // 8 + 4)
    return dict(particles=ps, global_ids=gid, partition=part, params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0 / 1200.0),
                colliders=colliders, cell_width=h, grid_capacity=max(1024, 1 << int(np.ceil(np.log2(nb * 1.5)))), model=model,
                global_particles=counts[0] * counts[1] * counts[2], name=name, bytes_per_particle=bpp)
