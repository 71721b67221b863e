"""-m gpu: particles removed at run time (include/wgsparkl_hip_remove.h). The truth needs no tolerance, as in tests/test_gpu_emit.py:
tests/test_gpu_bit_identity.py establishes checkpoint -> restart as bit-exact, so data that had particles removed must end bit for bit
where a twin ends that was created from the survivors' snapshot (their read_particles() rows in order, set_plastic_state, restored
colliders). Regions are held to tests/remove_truth.py on exactly representable coordinates, scheduled sinks to the explicit path: a twin
without sinks gets remove_particles_in by hand, in front of the scheduled substeps."""
import ctypes as C
import contextlib
from fractions import Fraction

import numpy as np
import pytest

import emit_truth as ET
import remove_truth as RT
from helpers import CDF_FIELDS, _digest, debug, new_data, pipeline, restored_colliders
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd.models import (MODEL_COROTATED, MODEL_FLUID, REGION_BALL, REGION_BOX, SINK_INSIDE, SINK_OUTSIDE, DruckerPrager, ElasticCoefficients,
                                 Emitter, FluidCoefficients, ForceField, ParticlePhase, Sink)
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider, ParticleSet, SimulationParams

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)
EVERY_FIELD = CDF_FIELDS + ("phase", "dp", "mass", "lambda_", "mu", "init_volume", "init_radius", "cdf_rigid_vel", "has_plasticity", "has_phase")


def assert_same_bits(a, b, fields, tag=None):
    """The same BITS field by field: fp32 fields are compared as their uint32 words (a NaN cdf normal equals itself)."""
    for f in fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        if x.dtype == np.float32 and y.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape and np.array_equal(x, y), f if tag is None else (tag, f)


def sub(ps, sel):
    return ParticleSet(**{k: (v[sel].copy() if isinstance(v, np.ndarray) else v) for k, v in ps.__dict__.items()})


def cat(*sets):
    return ParticleSet(**{k: (np.concatenate([getattr(s, k) for s in sets]) if isinstance(v, np.ndarray) else v) for k, v in sets[0].__dict__.items()})


def scene_of(ps, colliders=(), dt=1.0e-3, **kw):
    return dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0)[:ps.dim], dt=dt), colliders=list(colliders), cell_width=1.0,
                grid_capacity=4096, model=MODEL_COROTATED, **kw)


def floor(dim):
    return Collider.cuboid((1000.0, 2.0, 1000.0), (0.0, 0.0, 0.0)) if dim == 3 else Collider.cuboid((1000.0, 2.0), (0.0, 0.0), rotation=(0.0,))


def cloud(dim, n=1500, two_materials=True, seed=21, **kw):
    ps = scenes.random_cloud(n, dim=dim, seed=seed, extent=9.0, young=1.0e5, vel_scale=0.5, perturb_F=0.02, perturb_C=0.2,
                             phase=kw.pop("phase", ParticlePhase(1.0, FLT_MAX)), **kw)
    if two_materials:
        ps.lambda_[::2] *= np.float32(1.5)
    return ps


def block(dim, counts, plasticity=None, phase=ParticlePhase(1.0, FLT_MAX), origin=None, seed=5):
    """a lattice of ONE material (the uniform layouts take it)"""
    pos = scenes.lattice(counts[:dim], (origin or (6.0, 4.0, 6.0))[:dim], 1.0, 0.05, seed=seed)
    return ParticleSet.uniform(pos, 0.25, 1000.0, ElasticCoefficients.from_young_modulus(1.0e5, 0.3), plasticity=plasticity, phase=phase)


def assert_same_state(a, b, tag, models=False):
    pa, pb = a.read_particles(), b.read_particles()
    assert pa.n == pb.n, tag
    assert_same_bits(pa, pb, EVERY_FIELD, tag)
    assert _digest(a) == _digest(b), (tag, "digest")
    assert np.array_equal(a.read_positions().view(np.uint32), b.read_positions().view(np.uint32)), tag
    if models:
        assert np.array_equal(a.read_particle_models(), b.read_particle_models()), (tag, "models")


def random_mask(n, fraction, seed):
    return np.random.default_rng(seed).uniform(size=n) < fraction


def step_both(pipe, k, *datas):
    for d in datas:
        pipe.step(d, k)
        d.sync()


def restart_twin(sc, snap, bodies=None, **kw):
    """the twin created from a snapshot: its rows, its plastic state, the colliders where they are"""
    over = dict(particles=snap, **kw)
    if bodies is not None:
        over["colliders"] = restored_colliders(sc["colliders"], bodies, snap.dim)
    _, twin = new_data(sc, **over)
    if snap.n:
        twin.set_plastic_state(snap.dp_state)
    return twin


# ------------------------------------------------------------------------------------------------ 1. removed at substep 0 == created without them
def _dp_cloud(dim, mode):
    dp = DruckerPrager.new(1.0e6, 0.25)
    ps = cloud(dim, 1200, two_materials=False, plasticity=dp, phase=None, seed=23)
    rng = np.random.default_rng(4)
    if mode == 1:        # one set of h0..h3, the plasticity's lambda per particle
        ps.dp[:, 4] = (ps.dp[:, 4] * rng.uniform(0.9, 1.1, ps.n)).astype(np.float32)
    elif mode == 0:      # h0 per particle: the general layout
        ps.dp[:, 0] = (ps.dp[:, 0] * rng.uniform(0.9, 1.1, ps.n)).astype(np.float32)
    return scene_of(ps, [floor(dim)])


def _perturb_F(ps):
    ps.def_grad[:] = ps.def_grad + np.random.default_rng(17).normal(0.0, 0.01, ps.def_grad.shape).astype(np.float32)


def _case(name, dim, perturb=True):
    if name == "general":
        return scene_of(cloud(dim), [floor(dim)])
    if name == "uniform":
        return scene_of(block(dim, (14, 12, 10) if dim == 3 else (40, 30, 0)), [floor(dim)])
    if name.startswith("dp"):
        return _dp_cloud(dim, int(name[2]))
    if name == "fluid":
        ps = ParticleSet.uniform(scenes.lattice((12, 12, 8)[:dim] if dim == 3 else (30, 20), (8.3, 2.2, 8.0)[:dim], 1.0, 0.05), 0.25, 1000.0,
                                 FluidCoefficients(2.0e5, 0.0), phase=ParticlePhase(1.0, FLT_MAX))
        _perturb_F(ps)
        return {**scene_of(ps, [floor(dim)], dt=1.0 / 1200.0), "model": MODEL_FLUID, "fluid_gamma": 7.0}
    if name == "table":
        sc = scenes.block_in_fluid(dim, tank=(12, 8, 12) if dim == 3 else (30, 16), block=4)
        if perturb:
            _perturb_F(sc["particles"])
        perm = np.random.default_rng(8).permutation(sc["particles"].n)        # fluid and solid labels on both sides
        return {**sc, "particles": sub(sc["particles"], perm), "models": sc["models"][perm]}
    raise KeyError(name)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["general", "uniform", "dp2", "dp1", "dp0", "fluid", "table"])
def test_removed_at_substep_0_equals_created_without_them(hip_libs, name, dim):
    sc = _case(name, dim)
    ps, m = sc["particles"], sc.get("models")
    remove = random_mask(ps.n, 1.0 / 3.0, 100 + dim)
    keep = ~remove
    pipe, data = new_data(sc)
    kept_from = data.remove_particles(remove)
    assert np.array_equal(kept_from, RT.renumber(remove)[1]) and kept_from.dtype == np.uint32
    assert data.n == int(keep.sum()) == data.stats()["num_particles"]
    over = {"models": m[keep]} if m is not None else {}
    _, twin = new_data(sc, particles=sub(ps, keep), **over)
    if m is not None:
        assert (m[remove] == MODEL_FLUID).any() and (m[remove] != MODEL_FLUID).any() and (m[keep] == MODEL_FLUID).any()
    assert_same_state(data, twin, (name, dim, "before any substep"), models=True)
    step_both(pipe, 12, data, twin)
    assert_same_state(data, twin, (name, dim, "after 12 substeps"), models=True)
    assert data.diagnostics().num_nonfinite == 0


# ------------------------------------------------------------------------------------------------ 2. mid-run
def _mid_cases():
    yield "floor collider", scene_of(cloud(3, 1800), [floor(3)]), ()
    wb = scenes.walled_box(3, n=1800, speed=0.3)
    yield "walls and a force field", {**wb, "forces": [ForceField.uniform((0.0, -9.81, 0.0)), ForceField.vortex((10.0, 10.0, 10.0), 5.0)]}, ()
    yield "snow", scenes.snowball(3, radius=2.5), ()
    yield "REBIN_LAUNCH", scene_of(cloud(3, 1800, seed=31), [floor(3)]), ("REBIN_LAUNCH",)
    yield "NO_REBIN", scene_of(cloud(3, 1800, seed=32), [floor(3)]), ("NO_REBIN",)


@pytest.mark.parametrize("tag,sc,switches", list(_mid_cases()), ids=[c[0] for c in _mid_cases()])
def test_removed_mid_run_equals_a_restart_from_the_survivors(hip_libs, monkeypatch, tag, sc, switches):
    """Step 7, remove a third, step 13 against: the survivors' rows of the snapshot after 7 substeps, created anew with their plastic state
    and restored colliders, stepped 13."""
    with debug(monkeypatch, *switches) if switches else contextlib.nullcontext():
        ps = sc["particles"]
        pipe, data = new_data(sc)
        data.set_plastic_state(ps.dp_state)
        pipe.step(data, 7)
        data.sync()
        snap, bodies = data.read_particles(), data.read_body_poses()
        rebuilds = data.stats()["table_rebuilds"]
        remove = random_mask(ps.n, 1.0 / 3.0, 7)
        survivors = sub(snap, ~remove)
        kept_from = data.remove_particles(remove)
        assert np.array_equal(kept_from, np.flatnonzero(~remove))
        twin = restart_twin(sc, survivors, bodies)
        assert_same_bits(data.read_particles(), survivors, ("pos", "vel", "def_grad", "affine", "dp_state", "mass"), (tag, "read between the removal and the step"))
        step_both(pipe, 13, data, twin)
        assert data.stats()["table_rebuilds"] == rebuilds + 1, "the substep after the removal rebuilds the table, and no other"
        assert_same_state(data, twin, tag)
        assert data.diagnostics().num_nonfinite == 0 and data.stats()["substeps_done"] == 20


# ------------------------------------------------------------------------------------------------ 3. edges
N_EDGE = 700


def _pattern(name, n):
    remove = np.zeros(n, bool)
    if isinstance(name, int):
        remove[np.random.default_rng(300 + name).permutation(n)[:name]] = True
    elif name == "first":
        remove[0] = True
    elif name == "last":
        remove[-1] = True
    elif name == "every second":
        remove[::2] = True
    elif name == "all but one":
        remove[:] = True
        remove[n // 3] = False
    return remove


@pytest.mark.parametrize("pattern", [1, 63, 64, 65, "all but one", "first", "last", "every second"])
def test_removed_counts_around_a_wave_and_patterns(hip_libs, pattern):
    ps = cloud(3, N_EDGE, seed=41)
    sc = scene_of(ps, [floor(3)])
    pipe, data = new_data(sc)
    pipe.step(data, 2)
    data.sync()
    snap, bodies = data.read_particles(), data.read_body_poses()
    remove = _pattern(pattern, N_EDGE)
    kept_from = data.remove_particles(remove)
    assert np.array_equal(kept_from, RT.renumber(remove)[1]) and data.n == N_EDGE - int(remove.sum()) == data.stats()["num_particles"]
    twin = restart_twin(sc, sub(snap, ~remove), bodies)
    step_both(pipe, 3, data, twin)
    assert_same_state(data, twin, pattern)
    assert data.diagnostics().num_nonfinite == 0


def test_nothing_removed_leaves_no_trace_and_everything_removed_leaves_empty_data(hip_libs):
    ps = cloud(3, N_EDGE, seed=42)
    sc = scene_of(ps, [floor(3)])
    pipe, data = new_data(sc, particle_capacity=N_EDGE)
    _, plain = new_data(sc, particle_capacity=N_EDGE)
    step_both(pipe, 3, data, plain)
    before, stats = _digest(data), data.stats()
    kept_from = data.remove_particles(np.zeros(N_EDGE, bool))
    assert np.array_equal(kept_from, np.arange(N_EDGE)) and _digest(data) == before and data.stats() == stats and data.n == N_EDGE
    step_both(pipe, 4, data, plain)
    assert data.stats()["table_rebuilds"] == plain.stats()["table_rebuilds"] == stats["table_rebuilds"]
    assert_same_state(data, plain, "0 removed")
    # all of them: the data is empty, steps as empty data does, and takes the same records back like data created empty
    snap, bodies = data.read_particles(), data.read_body_poses()
    kept_from = data.remove_particles(np.ones(N_EDGE, bool))
    assert kept_from.shape == (0,) and data.n == 0 == data.stats()["num_particles"]
    assert data.read_positions().shape == (0, 3) and data.read_particles().n == 0 and data.diagnostics().num_particles == 0
    twin = restart_twin(sc, sub(snap, slice(0, 0)), bodies, particle_capacity=N_EDGE)
    step_both(pipe, 2, data, twin)
    for d in (data, twin):
        d.add_particles(snap)
    step_both(pipe, 4, data, twin)
    assert_same_bits(data.read_particles(), twin.read_particles(), EVERY_FIELD, "emptied, refilled")
    assert data.diagnostics().num_nonfinite == 0


def test_a_whole_cell_a_whole_block_and_two_removals_in_a_row(hip_libs):
    dense = block(3, (8, 8, 8), origin=(8.0, 8.0, 8.0))                      # one block (cells 8..11), 512 particles
    far = block(3, (4, 4, 4), origin=(8.0 + 80.0, 8.0, 8.0), seed=10)         # twenty blocks along x away
    sc = scene_of(cat(dense, far))
    pipe, data = new_data(sc)
    pipe.step(data, 4)
    data.sync()
    blocks_before = data.stats()["num_active_blocks"]
    snap = data.read_particles()
    cell = np.floor(snap.pos).astype(np.int64)
    in_cell = (cell == cell[100]).all(axis=1)                                 # every particle of one cell
    in_far = snap.pos[:, 0] > 50.0                                            # every particle of the far blocks
    assert 1 < in_cell.sum() < 30 and in_far.sum() == far.n
    k1 = data.remove_particles(in_cell)                                       # two removals without a step between them:
    k2 = data.remove_particles(in_far[~in_cell])                              # ... the second in the indices the first left
    keep = ~(in_cell | in_far)
    assert np.array_equal(k1[k2], np.flatnonzero(keep)) and data.n == int(keep.sum())
    twin = restart_twin(sc, sub(snap, keep))
    step_both(pipe, 6, data, twin)
    assert_same_state(data, twin, "a cell, the far blocks")
    assert data.stats()["num_active_blocks"] == twin.stats()["num_active_blocks"] < blocks_before, "the rebuild evicted the emptied blocks"


def test_remove_then_add_back_and_add_then_remove(hip_libs):
    ps = cloud(3, N_EDGE, seed=43)
    sc = scene_of(ps, [floor(3)])
    pipe, data = new_data(sc, particle_capacity=N_EDGE + 100)
    pipe.step(data, 3)
    data.sync()
    snap, bodies = data.read_particles(), data.read_body_poses()
    remove = random_mask(N_EDGE, 0.25, 44)
    data.remove_particles(remove)
    data.add_particles(sub(snap, remove))                                     # the same records, now behind the survivors
    union = cat(sub(snap, ~remove), sub(snap, remove))
    twin = restart_twin(sc, union, bodies, particle_capacity=N_EDGE + 100)
    assert_same_bits(data.read_particles(), union, ("pos", "vel", "def_grad", "affine", "mass", "lambda_", "mu", "dp_state"), "removed, added back: read")
    step_both(pipe, 5, data, twin)
    assert_same_state(data, twin, "removed, added back")
    # add, then remove some residents and some of the new ones, without a step between
    snap, bodies = data.read_particles(), data.read_body_poses()
    extra = sub(cloud(3, 100, seed=45), slice(0, 100))
    data.add_particles(extra)
    remove = random_mask(N_EDGE + 100, 0.3, 46)
    assert remove[:N_EDGE].any() and remove[N_EDGE:].any()
    data.remove_particles(remove)
    twin = restart_twin(sc, sub(cat(snap, extra), ~remove), bodies, particle_capacity=N_EDGE + 100)
    step_both(pipe, 5, data, twin)
    assert_same_state(data, twin, "added, removed")
    assert data.diagnostics().num_nonfinite == 0


def test_readers_between_the_removal_and_the_step_and_the_mass_sum(hip_libs):
    sc = _case("table", 3, perturb=False)
    n = sc["particles"].n
    pipe, data = new_data(sc)
    pipe.step(data, 5)
    data.sync()
    snap, models, fields, vb = data.read_particles(), data.read_particle_models(), data.particle_fields(), data.prep_vertex_buffer()
    remove = random_mask(n, 0.4, 47)
    keep = ~remove
    kept_from = data.remove_particles(remove)
    got = data.read_particles()
    assert got.n == int(keep.sum()) == data.n and np.array_equal(kept_from, np.flatnonzero(keep))
    assert_same_bits(got, sub(snap, keep), EVERY_FIELD + ("dp_state",), "the survivors, renumbered")
    assert np.array_equal(data.read_positions().view(np.uint32), snap.pos[keep].view(np.uint32))
    assert np.array_equal(data.read_particle_models(), models[keep])
    assert np.array_equal(data.prep_vertex_buffer().view(np.uint32), vb[keep].view(np.uint32))
    assert data.particle_fields().raw.tobytes() == fields.raw[keep].tobytes()
    diag = data.diagnostics()
    assert diag.num_particles == data.n == data.stats()["num_particles"] and diag.num_nonfinite == 0
    exact = lambda s: Fraction(int(s.fixed[0])) * Fraction(2) ** int(s.exponent)
    assert exact(diag.sums["mass"]) == sum(Fraction(float(m)) for m in snap.mass[keep]), "WGS_SUM_MASS is exactly the survivors'"


# ------------------------------------------------------------------------------------------------ 4. the keep-scan alone
TILE = 1024                      # kernels_remove.h REMOVE_TILE: ids per workgroup of the scan
TILES_PER_ROUND = 256            # ... and tile sums per round of the one workgroup that scans them


@pytest.mark.parametrize("n", [1, 63, TILE - 1, TILE, TILE + 1, TILE * TILES_PER_ROUND - 1, TILE * TILES_PER_ROUND, TILE * TILES_PER_ROUND + 1, 3 * TILE * TILES_PER_ROUND + 77])
def test_debug_compact_map_against_cumsum(hip_libs, n):
    lib, _ = hip_libs.load(3)
    pipe = pipeline(3)
    rng = np.random.default_rng(n)
    for name, remove in (("all keep", np.zeros(n, np.uint8)), ("none keep", np.full(n, 255, np.uint8)),
                         ("random", (rng.uniform(size=n) < 0.37).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8))):
        new_index, kept = np.full(n, 0xdeadbeef, np.uint32), C.c_uint32(0xdeadbeef)
        st = lib.wgs_debug_compact_map(pipe._h, remove.ctypes.data_as(C.POINTER(C.c_uint8)), n, new_index.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(kept))
        assert st == 0, lib.wgs_last_error()
        keep = remove == 0
        want = np.cumsum(keep, dtype=np.int64) - keep
        assert kept.value == int(keep.sum()), (name, n)
        assert np.array_equal(new_index, want.astype(np.uint32)), (name, n)
    assert lib.wgs_debug_compact_map(pipe._h, None, 0, None, None) == 0


# ------------------------------------------------------------------------------------------------ 5. regions
def _grid_particles(dim):
    """particles on multiples of 1/2 (3D: 13^3) or 1/4 (2D: 25^2) in [1, 7]: on, inside and outside every face used below, exactly"""
    step, m = (0.5, 13) if dim == 3 else (0.25, 25)
    axes = [1.0 + step * np.arange(m)] * dim
    pos = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, dim).astype(np.float32)
    return ParticleSet.uniform(pos, 0.25, 1000.0, ElasticCoefficients.from_young_modulus(1.0e5, 0.3), phase=ParticlePhase(1.0, FLT_MAX))


def _regions():
    box = Sink.box((4.0, 3.5, 4.5), (1.5, 1.0, 2.0))
    ball = Sink.ball((4.0, 4.0, 4.0), 2.5)                                    # (1.5, 2, 0) off the centre lies ON the sphere
    yield "box", [box]
    yield "ball", [ball]
    yield "outside box", [Sink.outside_box((4.0, 3.5, 4.5), (2.5, 2.0, 2.0))]
    yield "outside ball", [Sink(REGION_BALL, SINK_OUTSIDE, (4.0, 4.0, 4.0), (2.5, 0.0, 0.0))]
    yield "two overlapping", [ball, box]
    yield "a point", [Sink.box((2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), Sink.ball((3.0, 3.0, 3.0), 0.0)]


def _on_face(sink, pos):
    """the particles exactly on the region's boundary (the coordinates are exact in fp64)"""
    d = pos.astype(np.float64) - np.asarray(sink.center[:pos.shape[1]], np.float64)
    if sink.region == REGION_BOX:
        half = np.asarray(sink.half[:pos.shape[1]], np.float64)
        return (np.abs(d) <= half).all(axis=1) & (np.abs(d) == half).any(axis=1)
    return (d * d).sum(axis=1) == float(sink.half[0]) ** 2


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name,sinks", list(_regions()), ids=[r[0] for r in _regions()])
def test_regions_remove_exactly_what_the_truth_marks(hip_libs, name, sinks, dim):
    ps = _grid_particles(dim)
    sc = scene_of(ps)
    pipe, data = new_data(sc)
    pos = data.read_positions()
    assert np.array_equal(pos, ps.pos)
    remove, taker = RT.attribute(sinks, pos)
    assert remove.any() and (~remove).any() and _on_face(sinks[0], pos).any(), "the case has particles on a face, inside and outside"
    kept_from = data.remove_particles_in(sinks)
    assert np.array_equal(kept_from, RT.renumber(remove)[1]), name
    assert np.array_equal(data.read_positions(), pos[~remove]) and data.n == int((~remove).sum())
    # the mask forms give the same: the host mask, and the same mask in device memory with kept_from on the device
    import torch
    _, by_mask = new_data(sc)
    assert np.array_equal(by_mask.remove_particles(remove), kept_from)
    _, by_device = new_data(sc)
    mask_dev = torch.from_numpy(remove.astype(np.uint8)).to("cuda:0")
    kept_dev = torch.full((ps.n,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    assert by_device.remove_particles_device(mask_dev.data_ptr(), kept_dev.data_ptr()) == int(remove.sum())
    got = kept_dev.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:kept_from.size], kept_from) and (got[kept_from.size:] == 0xffffffff).all()
    step_both(pipe, 2, data, by_mask, by_device)
    assert_same_state(data, by_mask, (name, "regions == host mask"))
    assert_same_state(data, by_device, (name, "regions == device mask"))


@pytest.mark.parametrize("dim", [2, 3])
def test_an_outside_sink_takes_a_particle_with_a_nan_position(hip_libs, dim):
    ps = _grid_particles(dim)
    ps.pos[5, 1] = np.nan
    ps.pos[9, 0] = np.inf
    _, data = new_data(scene_of(ps))
    pos = data.read_positions()
    everything = Sink.box((4.0, 4.0, 4.0), (100.0, 100.0, 100.0))
    assert data.remove_particles_in([everything]).size == 2 and data.n == 2          # inside nothing: the box leaves the two
    assert np.array_equal(data.read_positions().view(np.uint32), pos[[5, 9]].view(np.uint32))
    _, data = new_data(scene_of(ps))
    outside = Sink.outside_box((4.0, 4.0, 4.0), (100.0, 100.0, 100.0))
    remove = RT.takes(outside, pos)
    assert list(np.flatnonzero(remove)) == [5, 9]
    assert np.array_equal(data.remove_particles_in([outside]), np.flatnonzero(~remove)) and data.n == ps.n - 2
    assert data.diagnostics().num_nonfinite == 0


# ------------------------------------------------------------------------------------------------ 6. sinks against the explicit path
def _two_emitters(dim, base):
    proto = sub(base, slice(3, 4))
    proto.vel[0] = (0.3, -2.0, 0.1)[:dim]
    proto2 = sub(base, slice(8, 9))
    proto2.vel[0] = (-0.5, -1.0, 0.4)[:dim]
    return [Emitter(proto, (3.0, 9.5, 3.0)[:dim], (3, 2, 3)[:dim], 0.5, jitter=0.3, seed=11, start_substep=1, period=3),
            Emitter(proto2, (6.0, 8.0, 5.0)[:dim], (2, 2, 2)[:dim], 0.45, jitter=0.0, seed=5, start_substep=0, period=5, batches=4)]


def _two_sinks():
    # a ball in the first emitter's lattice (it takes what was emitted before its pass), a box in the cloud; both due at substep 7
    return [Sink.ball((3.75, 10.0, 3.75), 0.75, start_substep=1, period=3), Sink.box((6.0, 5.0, 6.0), (1.25, 1.5, 1.25), start_substep=2, period=5)]


@pytest.mark.parametrize("dim,timestamps", [(3, False), (2, False), (3, True)])
def test_sinks_equal_the_explicit_path(hip_libs, dim, timestamps):
    base = cloud(dim, 900, seed=70 + dim)
    ems, sinks = _two_emitters(dim, base), _two_sinks()
    capacity = base.n + sum(ET.scheduled_batches(e, 24) * e.batch_size for e in ems)
    sc = scene_of(base, [floor(dim)])
    pipe, data = new_data(sc, particle_capacity=capacity, emitters=ems, sinks=sinks)
    assert [(k.region, k.side, k.center, k.half, k.start_substep, k.period) for k in data.sinks()] == [(k.region, k.side, k.center, k.half, k.start_substep, k.period) for k in sinks]
    device_bytes = data.stats()["device_bytes"]
    for k in (1, 5, 18):
        pipe.step(data, k, timestamps)
        data.sync()
        assert data.n == data.stats()["num_particles"]
    _, twin = new_data(sc, particle_capacity=capacity, emitters=ems)
    want = [0, 0]
    passes = 0
    for s in range(24):
        due = RT.due_sinks(sinks, s)
        if due:
            pos = twin.read_positions()
            for e, c in zip(due, RT.counts([sinks[e] for e in due], pos)):
                want[e] += c
            passes += 1
            kept_from = twin.remove_particles_in([sinks[e] for e in due])
            assert np.array_equal(kept_from, RT.renumber(RT.attribute([sinks[e] for e in due], pos)[0])[1]), s
        pipe.step(twin, 1)
    twin.sync()
    assert any(len(RT.due_sinks(sinks, s)) == 2 for s in range(24)) and passes == len({s for s in range(24) if RT.due_sinks(sinks, s)})
    assert data.sink_counts() == want and min(want) > 0, (data.sink_counts(), want)
    assert data.n == twin.n == data.stats()["num_particles"] == capacity - sum(want) - sum(data.emitter_counts()[1])
    assert data.emitter_counts() == twin.emitter_counts() and data.emitter_counts()[1] == [0, 0]
    assert data.stats()["device_bytes"] == device_bytes, "sinks take no device memory of the handle"
    assert_same_state(data, twin, ("sinks", dim, timestamps))
    assert data.stats()["table_rebuilds"] == twin.stats()["table_rebuilds"]
    if timestamps:
        assert data.read_timings()["grid sort"] > 0.0


def test_a_sink_that_catches_nothing_leaves_the_run_bit_identical(hip_libs):
    sc = scene_of(cloud(3, 900, seed=75), [floor(3)])
    nowhere = [Sink.box((500.0, 500.0, 500.0), (1.0, 1.0, 1.0), period=1), Sink.outside_box((0.0, 0.0, 0.0), (1.0e6, 1.0e6, 1.0e6), start_substep=3, period=2)]
    pipe, data = new_data(sc, sinks=nowhere)
    _, plain = new_data(sc)
    for k in (1, 7, 12):
        step_both(pipe, k, data, plain)
    assert data.sink_counts() == [0, 0] and data.n == plain.n == 900
    assert data.stats() == plain.stats()
    assert_same_state(data, plain, "a sink that catches nothing")


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_every_refusal_changes_nothing(hip_libs):
    lib, T = hip_libs.load(3)
    invalid, unsupported = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    sc = scene_of(block(3, (8, 8, 8)))
    pipe, data = new_data(sc)
    pipe.step(data, 2)
    data.sync()
    good = Sink.box((7.0, 5.0, 7.0), (0.5, 0.5, 0.5), start_substep=3, period=4)
    data.set_sinks([good])
    before, stats = _digest(data), data.stats()
    S = _ffi.Sink

    def raw(**fields):
        arr = (S * 1)()
        arr[0].region, arr[0].side, arr[0].start_substep, arr[0].period = good.region, good.side, good.start_substep, good.period
        arr[0].center[:], arr[0].half[:] = good.center, good.half
        for f, v in fields.items():
            if isinstance(v, tuple):
                getattr(arr[0], f)[v[0]] = v[1]
            else:
                setattr(arr[0], f, v)
        return arr

    removed, kept = C.c_uint32(77), (C.c_uint32 * 512)()
    mask = (C.c_uint8 * 512)(*([1] * 512))
    nine = (S * 9)()
    bad = [dict(region=0), dict(region=3), dict(side=2), dict(center=(0, float("nan"))), dict(center=(2, float("inf"))), dict(half=(1, -1.0)),
           dict(half=(0, float("nan"))), dict(half=(2, float("inf")))]
    for fields in bad:
        assert lib.wgs_set_sinks(data._h, raw(**fields), 1) == invalid, fields
        assert lib.wgs_remove_particles_in(data._h, raw(**fields), 1, kept, C.byref(removed)) == invalid, fields
        assert lib.wgs_last_error()
    # a ball reads half[0] alone; period is read by the setter alone
    assert lib.wgs_set_sinks(data._h, raw(period=0), 1) == invalid
    ball_ok = raw(region=REGION_BALL, half=(1, -1.0))
    ball_ok[0].center[:] = [500.0, 500.0, 500.0]
    everybody = (C.c_uint32 * 512)()
    assert lib.wgs_remove_particles_in(data._h, ball_ok, 1, everybody, C.byref(removed)) == 0 and removed.value == 0 and list(everybody) == list(range(512))
    removed.value = 77
    for call in (lambda: lib.wgs_set_sinks(data._h, nine, 9), lambda: lib.wgs_set_sinks(data._h, None, 1),
                 lambda: lib.wgs_remove_particles_in(data._h, nine, 9, kept, C.byref(removed)),
                 lambda: lib.wgs_remove_particles_in(data._h, None, 1, kept, C.byref(removed)),
                 lambda: lib.wgs_remove_particles_in(data._h, raw(), 1, kept, None),
                 lambda: lib.wgs_remove_particles(data._h, None, kept, C.byref(removed)),
                 lambda: lib.wgs_remove_particles(data._h, mask, kept, None),
                 lambda: lib.wgs_remove_particles(None, mask, kept, C.byref(removed)),
                 lambda: lib.wgs_remove_particles_device(data._h, None, None, C.byref(removed)),
                 lambda: lib.wgs_remove_particles_device(data._h, C.c_void_p(16), None, None),
                 lambda: lib.wgs_get_sinks(data._h, None, None), lambda: lib.wgs_get_sink_counts(data._h, None),
                 lambda: lib.wgs_get_sink_counts(None, (C.c_uint64 * 8)()),
                 lambda: lib.wgs_debug_compact_map(None, mask, 512, kept, None), lambda: lib.wgs_debug_compact_map(pipe._h, None, 512, kept, None)):
        assert call() == invalid
        assert lib.wgs_last_error()
    assert removed.value == 77 and list(kept) == [0] * 512
    with pytest.raises(ValueError):
        data.remove_particles(np.zeros(511, bool))
    assert data.sinks() == [good] and data.sink_counts() == [0], "the refusals left the set alone"
    assert _digest(data) == before and data.stats() == stats and data.n == 512
    data.set_sinks(None)
    assert data.sinks() == [] and data.sink_counts() == [] and _digest(data) == before and data.stats() == stats
    # sharded data
    slab_scene = scene_of(cloud(3, 600, two_materials=False, seed=90))
    shards, _ = lockstep_slabs(pipe, slab_scene, 2)
    cnt, n = (C.c_uint64 * 8)(), C.c_uint32(0)
    for s in shards:
        for call in (lambda: lib.wgs_remove_particles(s._h, mask, None, C.byref(removed)), lambda: lib.wgs_remove_particles_device(s._h, C.c_void_p(16), None, C.byref(removed)),
                     lambda: lib.wgs_remove_particles_in(s._h, raw(), 1, None, C.byref(removed)), lambda: lib.wgs_set_sinks(s._h, None, 0),
                     lambda: lib.wgs_set_sinks(s._h, raw(), 1)):
            assert call() == unsupported and b"single-domain data only" in lib.wgs_last_error()
        assert lib.wgs_get_sinks(s._h, (S * 8)(), C.byref(n)) == unsupported and lib.wgs_get_sink_counts(s._h, cnt) == unsupported


# ------------------------------------------------------------------------------------------------ 8. the scenes
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["drain", "channel"])
def test_the_scenes_run_at_a_bounded_particle_count(hip_libs, name, dim):
    """(tests/test_remove_abi.py shows on the CPU, with emit_truth and remove_truth, that the first batch is inside the sink after
    "transit_substeps" of free flight and that the capacity is twice the particles in flight)"""
    sc = getattr(scenes, name)(dim)
    em, sink = sc["emitters"][0], sc["sinks"][0]
    pipe, data = new_data(sc)
    assert data.n == 0 and data.particle_capacity == sc["particle_capacity"]
    substeps = 2 * sc["transit_substeps"] + 2 * sink.period
    for _ in range(4):
        pipe.step(data, substeps // 4)
        data.sync()
        assert data.n == data.stats()["num_particles"] < data.particle_capacity
    emitted, skipped = data.emitter_counts()
    assert skipped == [0] and emitted == [ET.scheduled_batches(em, 4 * (substeps // 4)) * em.batch_size]
    assert data.sink_counts()[0] > 0 and data.n == emitted[0] - data.sink_counts()[0]
    diag = data.diagnostics()
    assert diag.num_nonfinite == 0 and diag.num_particles == data.n
