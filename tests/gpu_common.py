"""Shared by the -m gpu test files: tolerances, seeded scenes, the oracle comparisons of block sets / particle fields / grid."""
from typing import NamedTuple

import numpy as np
import pytest

from wgsparkl_amd import MpmData, scenes
from wgsparkl_amd.models import (MODEL_COROTATED, MODEL_NEO_HOOKEAN, DruckerPrager, ElasticCoefficients, ParticlePhase)
from wgsparkl_amd.sharded import join_slabs, native_lockstep
from wgsparkl_amd.solver import Collider, ParticleSet, SimulationParams

import body_truth as BT
import cdf_truth as CT
import cpic_truth as CP
import mesh_truth as MT
import plastic_truth as PT
import transfer_truth as T
from helpers import (assert_close_to_truth, compare_cpic, compare_grids, grid_of, max_abs, new_data, pipeline, rel_rms, report_margin,
                     run_gpu, run_oracle)

GRID_V_TOL = 1e-5      # relative RMS of grid velocity vs the fp64 oracle (north_star target)
PART_TOL = 2e-5        # relative RMS of particle x, v, F, C' vs the fp64 oracle
# Collider (CPIC) scenes: discrete decisions (affinity / sign bits, det M > 1e-8, closest collider) sit on fp32
# thresholds, so a handful of particles may land on the other side; the comparison runs over the particles whose
# affinity bits agree, and the measured margins are reported (helpers.report_margin -> profiles/rNN_parity_margins.json)
CPIC_GRID_V_TOL = 5e-5
CPIC_PART_TOL = 5e-5
# fuzz scenes (random colliders of every kind, some dynamic, 12 substeps, against the fp32 oracle)
FUZZ_NODE_MISMATCH = 0.001     # measured: 0 in all 32 fuzz cases (profiles/r02_parity_margins.json)
FUZZ_PART_MISMATCH = 0.002     # measured: 0
FUZZ_VEL_TOL = 1e-4            # measured worst: 2.5e-5 (12 substeps of fp32 round-off growth through contact)
FUZZ_BODY_ATOL = 1e-4          # measured worst: 9.3e-6 (fixed-point impulses: 1e-5 resolution)


def cloud_scene(n=20000, dim=3, model=MODEL_COROTATED, seed=7, **kw):
    ps = scenes.random_cloud(n, dim=dim, seed=seed, phase=ParticlePhase(1.0, -1.0), **kw)
    g = (0.0, -9.81, 0.0)[:dim]
    return dict(particles=ps, params=SimulationParams(gravity=g, dt=1.0e-3), colliders=[], cell_width=1.0,
                grid_capacity=4096, model=model)


def check_blocks(data, st):
    vid, first, num, ids = data.read_blocks()
    ovid, ofirst, onum = st.blocks()
    assert np.array_equal(vid, ovid), "active block sets differ"
    assert np.array_equal(num, onum), "per-block particle counts differ"
    # sorted ids: same particles in each block (order inside a block is free in the reference)
    osorted = st.g["sorted_ids"][:st.n]
    of = st.g["first_particle"][:st.n_blocks]
    on = st.g["num_particles"][:st.n_blocks]
    ov = st.g["block_vid"][:st.n_blocks]
    oracle_sets = {tuple(ov[b]): frozenset(osorted[of[b]:of[b] + on[b]].tolist()) for b in range(st.n_blocks)}
    for b in range(len(vid)):
        got = frozenset(ids[first[b]:first[b] + num[b]].tolist())
        assert got == oracle_sets[tuple(vid[b])]
    assert sorted(ids.tolist()) == list(range(st.n))


def assert_runs_canonical(vid, first, num, ids, pos_before, dim, h):
    """The order the whole sort rests on, from read_blocks()'s arrays and the positions the sort saw: `ids` holds every
    particle once, and every block's run ids[first : first + num] goes by in-block cell (t0 + (t1 << BSHIFT) +
    (t2 << 2 BSHIFT), the cell being the one the cells-exact comparisons use: oracle.np_oracle.assoc_cell), the cells lying
    in the block, and by strictly ascending particle id inside a cell."""
    ids = np.asarray(ids, np.int64)
    n = len(pos_before)
    assert np.array_equal(np.sort(ids), np.arange(n)), "the sorted ids are not a permutation of the particles"
    assert int(np.asarray(num, np.int64).sum()) == n, "the runs do not hold every particle"
    bw = T.bw_of(dim)
    bshift = bw.bit_length() - 1
    cell = CT.assoc_cell(np.asarray(pos_before, np.float32), h)
    for b in range(len(vid)):
        run = ids[int(first[b]):int(first[b]) + int(num[b])]
        c = cell[run]
        assert np.array_equal(c // bw, np.broadcast_to(np.asarray(vid[b], np.int64), c.shape)), f"block {tuple(vid[b])}: a particle of its run is in another block"
        t = c % bw
        key = sum(t[:, k] << (bshift * k) for k in range(dim))
        step = np.diff(key)
        assert (step >= 0).all(), f"block {tuple(vid[b])}: the cells of its run do not ascend"
        assert (np.diff(run)[step == 0] > 0).all(), f"block {tuple(vid[b])}: ids do not ascend strictly inside a cell"


def assert_canonical_order(data, pos_before, dim, h):
    """assert_runs_canonical of what `data` holds after a substep; `pos_before`: the positions read BEFORE that substep (the
    sort of substep n orders the state substep n - 1 left)."""
    vid, first, num, ids = data.read_blocks()
    assert_runs_canonical(vid, first, num, ids, pos_before, dim, h)
    return vid, first, num, ids


class Checked(NamedTuple):
    """what checked_substep returns"""
    nodes: CT.NodeField            # the node truth of the substep
    particles: CT.ParticleField    # the end-to-end particle truth
    got: object                    # read_particles() after the substep
    rigid: object                  # the mesh_truth.Rigid of the substep (None without a mesh collider)


def checked_substep(tag, sc, data, fails, first, part_cap=CT.PART_CAP, colliders=None, before=None):
    """one substep of `data`, checked against the fp64 truth of the collider distance fields; `first`: the uploaded state is
    the state before it (else it is `before`, or read back). Where the scene has mesh colliders the truth includes the
    blocks and the votes of their samples (tests/mesh_truth.py); without one mesh_truth.rigid_of gives None and every step
    below is the analytic one."""
    ps = sc["particles"]
    d, h = ps.dim, sc["cell_width"]
    if first:
        pos, prev = ps.pos, ps.cdf_affinity
    else:
        before = data.read_particles() if before is None else before
        pos, prev = before.pos, before.cdf_affinity
    poses = data.read_body_poses()
    pipeline(d).step(data, 1)
    data.sync()
    cells, _, dist, aff, closest = data.read_grid()
    rg = MT.rigid_of(sc, poses, colliders)
    assert np.array_equal(cells, CT.active_cells(pos, h, d, rigid=rg)), f"{tag}: the active cells are not those of the positions"
    if rg is not None:
        assert not rg.und_blocks, f"{tag}: blocks whose membership depends on an undecided sample: {rg.und_blocks}"
    nf = CT.NodeField(CT.colliders_of(colliders or sc["colliders"], d, poses), d, h, cells, rigid=rg)
    CT.check_nodes(f"{tag} nodes", nf, dist, aff, closest, fails)
    got = data.read_particles()
    iso = CT.ParticleField(pos, h, cells, dist, aff, prev)
    CT.check_particle_cdf(f"{tag} isolated", iso, got.cdf_affinity, got.cdf_dist, got.cdf_normal, fails)
    e2e = CT.from_truth_nodes(pos, h, nf, prev)
    CT.check_particle_cdf(f"{tag} end to end", e2e, got.cdf_affinity, got.cdf_dist, got.cdf_normal, fails)
    CT.assert_caps(tag, nf, e2e, part_cap)
    return Checked(nf, e2e, got, rg)


class CheckedCpic(NamedTuple):
    """what checked_cpic_substep returns"""
    cdf: Checked                   # the distance-field check of the substep
    end_to_end: CP.Result          # the CPIC truth from the kernel's own decisions
    before: object                 # the particles before the substep
    got: object                    # ... and after it


def checked_cpic_substep(tag, sc, data, fails, first, part_cap=CT.PART_CAP, extra_levels=0.0):
    """one substep of `data` checked twice: the collider distance fields (checked_substep), and the CPIC transfer from the
    kernel's own read-back decisions (tests/cpic_truth.py): the particles' cdf fields, the nodes' affinities and closest
    ids, the bodies' velocities and centres of mass before the step. Every node's mass and velocity; every particle's x,
    v, F and C' from the kernel's own grid and end to end with the node bounds propagated."""
    ps = sc["particles"]
    d, h = ps.dim, sc["cell_width"]
    before = ps if first else data.read_particles()
    poses = data.read_body_poses()
    ck = checked_substep(tag, sc, data, fails, first, part_cap, before=before)
    cells, vm, _, aff, closest = data.read_grid()
    got = ck.got
    f = CP.Fields(got.cdf_affinity, got.cdf_normal.astype(np.float64), got.cdf_dist.astype(np.float64), cells, aff, closest)
    mo = CP.Motion.of(sc["colliders"], d, poses)
    inp = T.Inputs.of(before)
    prm = sc["params"]
    e2e = CP.substep(inp, h, prm.dt, prm.gravity, f, mo, extra_levels=extra_levels)
    near_n, nn, near_p = CP.check_result(f"{tag} cpic end to end", e2e, cells, vm, got, sc["model"], fails, extra_levels=extra_levels)
    iso = CP.substep(inp, h, prm.dt, prm.gravity, f, mo, own_grid=(cells, vm[:, :d]))
    CP.check_result(f"{tag} cpic isolated G2P", iso, None, None, got, sc["model"], fails)
    CP.assert_near(f"{tag} cpic", near_n, nn, near_p, inp.n)
    return CheckedCpic(ck, e2e, before, got)


class CheckedBodies(NamedTuple):
    """what checked_body_substep returns"""
    cpic: CheckedCpic              # the CPIC check of the substep
    impulses: BT.Impulses          # the interval of every body's accumulators, from the kernel's own decisions
    bodies: BT.BodyCheck           # the integration truth of every body and which outcome its state fits
    before: list                   # read_body_poses() before the substep
    after: list                    # ... and after it


def checked_body_substep(tag, sc, data, fails, first, part_cap=CT.PART_CAP, extra_levels=0.0):
    """one substep of `data` checked three times: checked_cpic_substep, and then what the bodies received and how they
    integrated (tests/body_truth.py): from the CPIC truth of the kernel's own decisions (its pairs, the read-back closest ids)
    and the poses read before the substep, the interval of every body's accumulators; from that interval, linvel, angvel,
    translation, rotation and com of every body read after the substep (wgs_step has flushed the integration by then). Asserts
    the sensitivity share of every body below the caps (body_truth.assert_sensitive)."""
    ps = sc["particles"]
    d, h, prm = ps.dim, sc["cell_width"], sc["params"]
    before = data.read_body_poses()
    ck = checked_cpic_substep(tag, sc, data, fails, first, part_cap, extra_levels)
    after = data.read_body_poses()
    mo = CP.Motion.of(sc["colliders"], d, before)
    imp = BT.impulses(ck.end_to_end, T.Inputs.of(ck.before), mo)
    bodies = BT.check_bodies(f"{tag} bodies", imp, BT.Props(sc["colliders"], d), before, after, h, prm.dt, prm.gravity, fails)
    report_margin(f"{tag}: bodies near a cap (share)", bodies.near / max(len(after), 1), BT.NEAR_MAX, count=bodies.near)
    # a condition on the inputs, whatever the scene: every node that gives a body below the caps an impulse is visible in its velocity
    BT.assert_sensitive(tag, bodies)
    return CheckedBodies(ck, imp, bodies, before, after)


UNTOUCHED = ("lambda_", "mu", "dp", "init_volume")     # what a plastic substep leaves bit for bit


def _start(sc, **kw):
    """data of a scene with the plastic state of its particles (creation takes none: set_plastic_state); `kw` as in new_data"""
    pipe, data = new_data(sc, **kw)
    data.set_plastic_state(kw.get("particles", sc["particles"]).dp_state)
    return pipe, data


def _step(pipe, data, k=1):
    pipe.step(data, k)
    data.sync()
    return data.read_particles()


def plastic_twin(sc, particles=None):
    """one substep of the scene (or of a read-back state of it) stripped of plasticity (plastic_truth.strip), whatever its rule"""
    return _step(*_start(PT.strip(sc, particles=particles), plasticity=None))


class CheckedPlastic(NamedTuple):
    """what checked_plastic_substep returns"""
    end_to_end: object             # the particle truth of the trial state (transfer_truth.Particles), end to end
    isolated: object               # ... from the kernel's own grid
    keep: object                   # the particles the collider leaves to the particle checks (None without colliders: all)


def checked_plastic_substep(tag, sc, before, got, twin, grid, poses, model, fails, extra_levels=0.0):
    """What one substep of plastic particles is held to before its plasticity rule is looked at, from the state `before` (a ParticleSet
    with its dp_state and phase) to `got`, with `twin` the stripped run's result, `grid` the read_grid() after the substep and
    `poses` the bodies read before it (None without colliders; with them the trial state is cpic_truth's, from the kernel's own
    decisions, as in checked_cpic_substep): UNTOUCHED bit for bit, the twin's x and v the plastic run's, every node, the twin's
    particles from the kernel's own grid, and the shares near the clamp and the speed cap under plastic_truth.NEAR_MAX."""
    d, h, prm, n = before.dim, sc["cell_width"], sc["params"], before.n
    inp = T.Inputs.of(before)
    cells, vm = grid[:2]
    for k in UNTOUCHED:
        assert np.array_equal(getattr(got, k), getattr(before, k)), f"{tag}: {k} changed"
    assert np.array_equal(twin.pos, got.pos) and np.array_equal(twin.vel, got.vel), f"{tag}: the elastic twin's x or v differ from the plastic run's"
    if sc["colliders"]:
        f = CP.Fields(got.cdf_affinity, got.cdf_normal.astype(np.float64), got.cdf_dist.astype(np.float64), cells, grid[3], grid[4])
        mo = CP.Motion.of(sc["colliders"], d, poses)
        e2e = CP.substep(inp, h, prm.dt, prm.gravity, f, mo, extra_levels=extra_levels)
        near_n, nn = T.check_grid(f"{tag} grid", e2e.grid, cells, vm, fails, extra_levels=extra_levels)
        pt = e2e.particles
        iso = CP.substep(inp, h, prm.dt, prm.gravity, f, mo, own_grid=(cells, vm[:, :d])).particles
        keep = ~e2e.contact.near_pen
        near_p = int((pt.near_cap | e2e.contact.near).sum())
        assert (got.cdf_affinity != 0).sum() > 0.02 * n, f"{tag}: the collider is not felt by the cloud"
    else:
        st, gr, pt = T.substep(inp, h, prm.dt, prm.gravity, extra_levels=extra_levels)
        near_n, nn = T.check_grid(f"{tag} grid", gr, cells, vm, fails, extra_levels=extra_levels)
        iso = T.isolated(inp, st, cells, vm[:, :d], prm.dt)
        keep = None
        near_p = int(pt.near_cap.sum())
    # the elastic twin: its def_grad is the kernel's own F_trial
    T.check_particles(f"{tag} twin isolated G2P", iso, twin, model, fails, sel=keep)
    report_margin(f"{tag}: nodes near the clamp (fraction)", near_n / max(nn, 1), PT.NEAR_MAX, count=near_n)
    report_margin(f"{tag}: particles near the speed cap (fraction)", near_p / n, PT.NEAR_MAX, count=near_p)
    assert near_n <= PT.NEAR_MAX * nn and near_p <= PT.NEAR_MAX * n
    return CheckedPlastic(pt, iso, keep)


class SteadyPlastic(NamedTuple):
    """what steady_plastic_substep returns"""
    before: object                 # read_particles() after the warm-up
    got: object                    # ... and after the checked substep
    twin: object                   # the checked substep of new data made of `before` without plasticity
    grid: tuple                    # read_grid() after the checked substep
    stats0: dict                   # stats() before the checked substep
    stats1: dict                   # ... and after it


def steady_plastic_substep(sc, warmup):
    """`warmup` substeps, read back (plastic state and phase included), then one more: a steady-state substep, which rebuilds no table
    and in which some particle changes its cell. The twin is new data made of the read-back state without plasticity (a restart
    continues bit for bit)."""
    pipe, data = _start(sc)
    before = _step(pipe, data, warmup)
    s0 = data.stats()
    got = _step(pipe, data)
    s1 = data.stats()
    grid = data.read_grid()
    twin = plastic_twin(sc, particles=before)
    assert s1["table_rebuilds"] == s0["table_rebuilds"], "the checked substep rebuilt the table: not a steady-state substep"
    assert s1["cell_changers"] > s0["cell_changers"], "no particle changed cell in the checked substep"
    return SteadyPlastic(before, got, twin, grid, s0, s1)


def blocks_in_reach(nf, col, d):
    """the blocks that hold a node at which collider `col` votes"""
    return set(map(tuple, np.unique(nf.cells[nf.voter[:, col]] // T.bw_of(d), axis=0).tolist()))


def check_fields(data, st32, st64, tol=PART_TOL):
    got = data.read_particles()
    for name in ("pos", "vel", "def_grad", "affine"):
        assert_close_to_truth(name, getattr(got, name), st32.arr[name], st64.arr[name], tol)
    return got


def check_grid(data, st32, st64, dim=3):
    gv, ov = compare_grids(data.read_grid(), grid_of(st64))
    o32 = grid_of(st32)[1]
    assert_close_to_truth("grid velocity", gv[:, :dim], o32[:, :dim], ov[:, :dim], GRID_V_TOL)
    assert_close_to_truth("grid mass", gv[:, dim], o32[:, dim], ov[:, dim], GRID_V_TOL)


def _exploding_cube():
    sc = scenes.neo_hookean_cube(n_side=8)
    ps = sc["particles"]
    c = ps.pos.mean(0)
    ps.vel[:] = ((ps.pos - c) * 25.0).astype(np.float32)       # radial: the cube flies apart
    ps.lambda_[:] = 1.0                                         # (next to no stiffness: nothing holds it together)
    ps.mu[:] = 1.0
    sc["params"] = SimulationParams(gravity=(0.0, 0.0, 0.0), dt=sc["params"].dt)
    return sc


def _random_scene(seed):
    """Seeded random configuration: dimension, material / plasticity, 0-3 colliders of random kind (ball, cuboid,
    capsule, mesh), pose and motion, some of them dynamic."""
    rng = np.random.default_rng(1000 + seed)
    dim = 3 if seed % 2 == 0 else 2
    plastic = DruckerPrager.new(1e6, 0.25) if rng.random() < 0.4 else None
    phase = None if (plastic is not None and rng.random() < 0.5) else ParticlePhase(1.0, -1.0)
    ps = scenes.random_cloud(1200, dim=dim, seed=100 + seed, extent=9.0, young=1e6, plasticity=plastic, phase=phase,
                             vel_scale=1.5, perturb_F=0.02, perturb_C=0.2)
    cols = []
    for _ in range(int(rng.integers(0, 4))):
        kind = int(rng.integers(0, 4))
        pos = tuple(float(x) for x in rng.uniform(1.0, 9.0, dim))
        vel = tuple(float(x) for x in rng.uniform(-1.0, 1.0, 3))
        if dim == 3:
            axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
            ang = float(rng.uniform(0, 1.5))
            rot = tuple(float(x) for x in np.append(axis * np.sin(ang / 2), np.cos(ang / 2)))
            angvel = tuple(float(x) for x in rng.uniform(-0.8, 0.8, 3))
        else:
            rot = (float(rng.uniform(0, 1.5)),)
            angvel = (float(rng.uniform(-0.8, 0.8)),)
        kw = dict(rotation=rot, linvel=vel, angvel=angvel)
        if kind == 0:
            c = Collider.ball(float(rng.uniform(0.8, 2.0)), pos, **kw)
        elif kind == 1:
            c = Collider.cuboid(tuple(float(x) for x in rng.uniform(0.6, 2.5, dim)), pos, **kw)
        elif kind == 2:
            c = Collider(2, (float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.4, 1.0))), pos, **kw)   # capsule
        elif dim == 3:
            v = np.array([[-2.3, 0.1, -2.1], [-2.2, 0.0, 2.4], [2.1, 0.3, -2.2], [2.4, -0.2, 2.3]], np.float32)
            c = Collider.trimesh(v, np.array([[0, 1, 2], [2, 1, 3]]), pos, **kw)
        else:
            v = np.array([[-3.1, 0.2], [-0.4, -0.3], [2.9, 0.4]], np.float32)
            c = Collider.polyline(v, np.array([[0, 1], [1, 2]]), pos, **kw)
        if kind in (0, 1) and rng.random() < 0.5:
            c = c.with_density(float(rng.uniform(5.0, 50.0)), dim)
        cols.append(c)
    g = (0.0, -9.81, 0.0)[:dim]
    return dict(particles=ps, params=SimulationParams(gravity=g, dt=8e-4), colliders=cols, cell_width=1.0,
                grid_capacity=2048, model=int(rng.integers(0, 2)))


def _bed_scene(d, h, n=None, drift=0.0):
    """a bed of `n` particles 6 blocks long whose lowest half cell lies inside a fixed floor, stirred (a swirl of 0.15 h / dt
    plus noise, plus `drift` h / dt along x), and a kinematic ball driven into its top at 0.09 h per substep"""
    bw = T.bw_of(d)
    rng = np.random.default_rng(60 + d)
    floor = Collider.cuboid(CT._v(np.array([3.2 * bw, 1.0, 3.0 * bw]) * h, d), CT._v(np.array([3.0 * bw + 0.13, bw - 0.8, 1.5 * bw + 0.21]) * h, d),
                            rotation=CT.ident(d))
    lin = np.zeros(3)
    lin[:d] = (np.array([0.03, -0.08, 0.02]) * h / T.DT)[:d]
    ball = Collider.ball(float(np.float32(1.5 * h)), CT._v(np.array([3 * bw + 0.4, 2 * bw + 3.6, 1.5 * bw + 0.27]) * h, d),
                         linvel=tuple(float(v) for v in CT.f32(lin)), angvel=(0.7,) if d == 2 else (0.3, -0.5, 0.4))
    lo, hi = np.array([1.0, bw - 0.3, bw + 0.5]) * h, np.array([6 * bw - 1.0, 2 * bw + 3.0, 2 * bw + 2.5]) * h
    sc = CT._static(d, h, rng, [floor, ball], [(lo, hi)], n or (3000 if d == 3 else 1500), rim_keep=1.0)
    ps = sc["particles"]
    c = ps.pos.mean(0)
    vel = np.zeros((ps.n, d))
    vel[:, 0] = -(ps.pos[:, 1] - c[1])
    vel[:, 1] = ps.pos[:, 0] - c[0]
    vel = vel * (0.15 * h / T.DT / (3.0 * bw * h)) + rng.normal(0.0, 0.03 * h / T.DT, (ps.n, d))
    vel[:, 0] += drift * h / T.DT
    ps.vel[:] = vel.astype(np.float32)
    sc["params"] = SimulationParams(gravity=T.GRAVITY[:d], dt=T.DT)
    return sc


def _joined_with_cdf(shards, n):
    """sharded.join_slabs of every slab's state and cdf, every particle exactly once; and (cdf_affinity, cdf_dist, cdf_normal) in the
    same order under the one rule that is not the record's: a cdf whose stamp is not the newest stamp is the default cdf"""
    joined = join_slabs([s.export(cdf=True) for s in shards], np.arange(n))
    assert joined.exact, joined.problem
    f = joined.fields
    live = f["cdf_stamp"] == f["cdf_stamp"].max()
    return joined, (np.where(live, f["cdf_affinity"], 0).astype(np.uint32), np.where(live, f["cdf_dist"], 0.0),
                    np.where(live[:, None], f["cdf_normal"], 0.0))


def _export_all(shards, n, d):
    """(pos, cdf_affinity, cdf_dist, cdf_normal) of the particles of all slabs in the order of their global ids"""
    joined, cdf = _joined_with_cdf(shards, n)
    return (joined.fields["pos"],) + cdf


def export_state_and_cdf(shards, n, d):
    """({pos, vel, def_grad, affine, mass} in the order of the global ids, the rank that holds each particle, cdf_affinity, cdf_dist,
    cdf_normal), from one export per slab"""
    joined, cdf = _joined_with_cdf(shards, n)
    return ({f: joined.fields[f] for f in ("pos", "vel", "def_grad", "affine", "mass")}, joined.holder) + cdf


def check_lockstep_slabs(tag, sc, shards, part, nsteps, fails):
    """`nsteps` lockstep substeps of the scene's two slabs (sharded.lockstep_slabs), each with the poses read before it: every particle
    against the truth of the whole domain (the samples of a mesh collider included; without one mesh_truth.rigid_of gives
    None), the nodes of each slab's own blocks against the truth restricted to them, and no collider-affine node of a
    slab's range missing from its grid. Returns, per substep, whether collider 1 votes at a node past the cut."""
    ps = sc["particles"]
    d, h = ps.dim, sc["cell_width"]
    bw = T.bw_of(d)
    ranges = [part.block_range(r) for r in range(len(shards))]
    cut = ranges[1][0]
    pos, prev = ps.pos, np.zeros(ps.n, np.uint32)
    crossed = []
    for k in range(nsteps):
        poses = shards[0].read_body_poses()
        native_lockstep(shards[0].pipeline, shards, 1)
        for s in shards:
            s.sync()
        cols = CT.colliders_of(sc["colliders"], d, poses)
        tag_k = f"{tag} substep {k}"
        rg = MT.rigid_of(sc, poses)
        whole = CT.NodeField(cols, d, h, CT.active_cells(pos, h, d, rigid=rg), rigid=rg)
        if rg is not None:
            assert not rg.und_blocks
        e2e = CT.from_truth_nodes(pos, h, whole, prev)
        npos, aff, dist, normal = _export_all(shards, ps.n, d)
        CT.check_particle_cdf(f"{tag_k} end to end", e2e, aff, dist, normal, fails)
        CT.assert_caps(tag_k, whole, e2e)
        for r, s in enumerate(shards):
            cells, _, ndist, naff, nclosest = s.read_grid()
            blk = cells[:, 0] // bw
            own = (blk >= ranges[r][0]) & (blk < ranges[r][1])
            assert own.any()
            nf = CT.NodeField(cols, d, h, cells[own], rigid=rg)       # (the samples' own blocks: those of the whole domain)
            CT.check_nodes(f"{tag_k} slab {r} own nodes", nf, ndist[own], naff[own], nclosest[own], fails)
            inside = set(map(tuple, cells[own].tolist()))
            missing = [c for c in whole.cells[(whole.aff != 0) & (whole.cells[:, 0] // bw >= ranges[r][0]) & (whole.cells[:, 0] // bw < ranges[r][1])].tolist()
                       if tuple(c) not in inside]
            assert not missing, f"{tag_k} slab {r}: {len(missing)} collider-affine nodes of its range are not in its grid"
        crossed.append(bool((whole.voter[:, 1] & (whole.cells[:, 0] >= cut * bw)).any()))
        pos, prev = npos, aff
    return crossed
