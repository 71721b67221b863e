"""-m gpu: per-particle constitutive models (MpmData.set_particle_models) on the device — uniform tables against the global models,
separated bodies against each body alone, coupled fluid + solid bodies against the fp64 truth of tests/mixed_truth.py, launch shapes,
the label's journey through the sort and a restart, diagnostics and drawing, argument checks.

Figures measured on one MI355X are in profiles/r11_mixed_margins.json (every comparison goes through helpers.report_margin)."""
import contextlib
import ctypes as C
import dataclasses
import math
import types

import numpy as np
import pytest

import diag_truth as dt_
import fluid_truth as ft
import mixed_truth as mt
from gpu_common import GRID_V_TOL, PART_TOL
from helpers import BASE_FIELDS, _digest, assert_close_to_truth, assert_same_bits, debug, new_data, pipeline, report_margin
from oracle import np_oracle
from test_gpu_fluid import ELASTIC_ROUNDINGS, FIELDS, SHAPES
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd._ffi import WgsError
from wgsparkl_amd.models import (MODEL_COROTATED, MODEL_FLUID, MODEL_NEO_HOOKEAN, MODEL_PER_PARTICLE, DruckerPrager, ElasticCoefficients,
                                 FluidCoefficients, ParticlePhase)
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider, ParticleSet, SimulationParams

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ARRAYS = [f.name for f in dataclasses.fields(ParticleSet) if f.name != "dim"]


def _run(sc, calls=(15, 15), **overrides):
    _, data = new_data(sc, **overrides)
    for k in calls:
        data.pipeline.step(data, k)
    data.sync()
    return data


def _assert_same_particles(a, b, what=""):
    """bit for bit (by the bytes: a NaN equals itself here — the cdf normal of a particle wedged between opposite faces is 0 / 0)"""
    for f in ARRAYS:
        x, y = np.ascontiguousarray(getattr(a, f)), np.ascontiguousarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, f)


def _assert_same_state(a, b, what=""):
    """every field of read_particles, read_grid and the digest"""
    _assert_same_particles(a.read_particles(), b.read_particles(), what)
    for k, (x, y) in enumerate(zip(a.read_grid(), b.read_grid())):
        assert np.array_equal(x, y), (what, "grid", k)
    assert _digest(a) == _digest(b), what


def _landing_block(dim, seed=6):
    """A jittered elastic block falling onto the floor cuboid: its lowest layers are near the collider from the first substep."""
    h = 1.0
    counts = (16, 16, 16) if dim == 3 else (40, 40)
    pos = scenes.lattice(counts, (9.0, 2.3, 9.0)[:dim], h, 0.05, seed=seed)
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, ElasticCoefficients.from_young_modulus(2.0e5, 0.3), phase=ParticlePhase(1.0, scenes.FLT_MAX))
    ps.vel[:, 1] = -6.0
    ps.vel[:, 0] = ((pos[:, 1] - pos[:, 1].mean()) * 2.0).astype(np.float32)
    floor = Collider.cuboid((1000.0, 2.0, 1000.0), (0.0, 0.0, 0.0)) if dim == 3 else Collider.cuboid((1000.0, 1.0), (0.0, 1.0), rotation=(0.0,))
    return dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0), colliders=[floor], cell_width=h,
                grid_capacity=4096, model=MODEL_COROTATED, fluid_gamma=7.0)


def _tank(dim):
    """All fluid, near colliders: the dam break in 3D, the tank of block_in_fluid (without its block's label) in 2D."""
    if dim == 3:
        return scenes.dam_break(viscosity=5.0)
    sc = scenes.block_in_fluid(dim=2, tank=(40, 24), block=8, gap=0.1, drop_speed=8.0)
    ps = sc["particles"]
    solid = sc["models"] != MODEL_FLUID
    ps.lambda_[solid], ps.mu[solid] = ps.lambda_[0], ps.mu[0]
    del sc["models"]
    return sc


# ------------------------------------------------------------------------------------------------ 1. uniform tables
@pytest.mark.parametrize("switch", [(), ("NO_UNIFORM",)])
@pytest.mark.parametrize("m", [MODEL_COROTATED, MODEL_NEO_HOOKEAN, MODEL_FLUID])
@pytest.mark.parametrize("dim", [3, 2])
def test_uniform_table_is_the_global_model(hip_libs, monkeypatch, dim, m, switch):
    """A table that labels every particle m and wgs_set_constitutive_model(m): the same bits in every field of read_particles and
    read_grid and the same digest after 30 substeps over two calls — the mixed kernel's branch for m is m's own kernel."""
    with debug(monkeypatch, *switch) if switch else contextlib.nullcontext():
        make = (lambda: _tank(dim)) if m == MODEL_FLUID else (lambda: _landing_block(dim))
        sc = make()
        ref = _run(sc, model=m)
        sc2 = dict(make(), models=np.full(sc["particles"].n, m, np.uint8))
        got = _run(sc2, model=MODEL_COROTATED if m != MODEL_COROTATED else MODEL_NEO_HOOKEAN)   # (the data's own model is another one)
        _assert_same_state(ref, got, (dim, m, switch))
        assert got.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_PER_PARTICLE and ref.diagnostics(_ffi.DIAG_PARTICLES).model == m
        p = got.read_particles()
        assert (p.cdf_affinity != 0).sum() > 50, "the scene should touch its colliders"
        assert np.isfinite(p.pos).all() and np.isfinite(p.affine).all() and got.stats()["overflow"] == 0


# ------------------------------------------------------------------------------------------------ 2. separated bodies
def _body(dim, k, x0):
    h = 1.0
    counts = (8, 8, 8) if dim == 3 else (16, 16)
    pos = scenes.lattice(counts, (x0, 9.0, 9.0)[:dim], h, 0.05, seed=20 + k)
    mat = (ElasticCoefficients.from_young_modulus(2.0e5, 0.3), ElasticCoefficients.from_young_modulus(3.0e5, 0.25), FluidCoefficients(1.5e5, 8.0))[k]
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, mat, phase=ParticlePhase(1.0, scenes.FLT_MAX))
    c = pos.mean(0)
    ps.vel[:] = ((c - pos) * 2.5).astype(np.float32)
    ps.vel[:, 0] += ((pos[:, 1] - c[1]) * 3.0).astype(np.float32)
    return ps


def _concat(sets):
    kw = {f: np.concatenate([getattr(s, f) for s in sets]) for f in ARRAYS}
    return ParticleSet(dim=sets[0].dim, **kw)


@pytest.mark.parametrize("dim", [3, 2])
def test_separated_bodies_equal_each_body_alone(hip_libs, dim):
    """Three bodies — corotated, neo-Hookean, fluid, each with its own lambda / mu — at least three blocks apart along x (no shared active block),
    in free fall with converging velocities: in one simulation under a table, every particle ends with the bits it ends with when its
    body runs alone under the global model. Ids ascend within a body in both runs (the canonical summation order is by id)."""
    gap = 20.0 if dim == 3 else 40.0                       # blocks are 4 cells wide in 3D, 8 in 2D; a body spans 4 / 8 cells
    bodies = [_body(dim, k, 9.0 + gap * k) for k in range(3)]
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0)
    base = dict(params=params, colliders=[], cell_width=1.0, grid_capacity=4096, fluid_gamma=5.0)
    models = np.concatenate([np.full(b.n, k, np.uint8) for k, b in enumerate(bodies)])
    data = _run(dict(base, particles=_concat(bodies), models=models, model=MODEL_COROTATED))
    both, vid = data.read_particles(), data.read_blocks()[0]
    xs = np.unique(vid[:, 0])
    assert np.sum(np.diff(xs) >= 3) == 2, "the bodies must be at least three blocks apart"
    lo = 0
    for k, b in enumerate(bodies):
        alone = _run(dict(base, particles=b, model=k)).read_particles()
        assert_same_bits(types.SimpleNamespace(**{f: getattr(both, f)[lo:lo + b.n] for f in BASE_FIELDS}), alone, BASE_FIELDS, k)
        assert np.abs(alone.def_grad - np.eye(dim, dtype=np.float32).reshape(-1)).max() > 0.02
        lo += b.n


# ------------------------------------------------------------------------------------------------ 3. coupled parity
@pytest.mark.parametrize("pattern", mt.PATTERNS)
@pytest.mark.parametrize("solid_model", [MODEL_COROTATED, MODEL_NEO_HOOKEAN])
@pytest.mark.parametrize("dim", [3, 2])
def test_coupled_parity_with_the_fp64_truth(hip_libs, dim, solid_model, pattern):
    """Fluid and solid in one body, 24 substeps over two calls: blocks, counts and node cells exact by virtual id; grid velocity / mass,
    position, velocity, F of the solid rows, J of the fluid rows and `affine` within GRID_V_TOL / PART_TOL of the fp64 MixedState
    (ref32 = its fp32 run; test_mixed_truth.py holds the scenes to half of these bounds). Fluid rows keep diag(J, 1[, 1]) exactly."""
    sc, s64, s32 = mt.coupled_truths(dim, solid_model, pattern)
    fl = sc["fluid"]
    ps = sc["particles"]
    data = _run(sc, (12, 12))
    assert mt.SUBSTEPS == 24
    tag = f"mixed {dim}D solid={solid_model} {pattern}"
    vid, first, num, ids = data.read_blocks()
    tv, tn = s64.active_blocks()
    assert np.array_equal(vid, tv), "active block sets differ"
    assert np.array_equal(num, tn), "per-block particle counts differ"
    assert sorted(ids.tolist()) == list(range(ps.n))
    cells, vm = data.read_grid()[:2]
    tc, tvm = s64.grid_records()
    assert np.array_equal(cells, tc), "active node cells differ"
    v32, m32 = s32.grid_at(tc.astype(np.int64))
    assert_close_to_truth(f"{tag}: grid velocity", vm[:, :dim], v32, tvm[:, :dim], GRID_V_TOL)
    assert_close_to_truth(f"{tag}: grid mass", vm[:, dim], m32, tvm[:, dim], GRID_V_TOL)
    got = data.read_particles()
    eye = np.eye(dim, dtype=np.float32).reshape(-1)
    assert np.array_equal(got.def_grad[fl][:, 1:], np.tile(eye[1:], (int(fl.sum()), 1)))
    assert_close_to_truth(f"{tag}: pos", got.pos, s32.pos, s64.pos, PART_TOL)
    assert_close_to_truth(f"{tag}: vel", got.vel, s32.vel, s64.vel, PART_TOL)
    assert_close_to_truth(f"{tag}: J (fluid rows)", got.def_grad[fl][:, 0], s32.J[fl], s64.J[fl], PART_TOL)
    assert_close_to_truth(f"{tag}: F (solid rows)", got.def_grad[~fl], s32.F[~fl], s64.F[~fl], PART_TOL)
    assert_close_to_truth(f"affine ({tag})", got.affine, s32.C, s64.C, PART_TOL)
    assert np.array_equal(got.lambda_, ps.lambda_) and np.array_equal(got.mu, ps.mu) and np.array_equal(got.mass, ps.mass)
    assert np.array_equal(data.read_particle_models(), sc["models"])
    assert data.stats()["overflow"] == 0


# ------------------------------------------------------------------------------------------------ 4. / 5. launch shapes, the label, restart
def _drop(dim=3, solid_model=MODEL_NEO_HOOKEAN):
    if dim == 3:
        return scenes.block_in_fluid(dim=3, tank=(24, 12, 16), block=8, gap=0.1, drop_speed=10.0, viscosity=5.0, solid_model=solid_model)
    return scenes.block_in_fluid(dim=2, tank=(40, 24), block=12, gap=0.1, drop_speed=10.0, viscosity=5.0, solid_model=solid_model)


@pytest.mark.parametrize("dim,solid_model", [(3, MODEL_NEO_HOOKEAN), (2, MODEL_COROTATED)])
def test_launch_shapes_and_runs_are_bit_identical(hip_libs, monkeypatch, dim, solid_model):
    """An elastic block dropped into a tank of Tait fluid (floor and walls: the list walk and the CPIC paths advance both kinds): the
    default run twice and under each launch-shape switch of test_gpu_fluid.py — the same bits; the label arrives with its particle."""
    ref = None
    for names in SHAPES:
        with debug(monkeypatch, *names) if names else contextlib.nullcontext():
            sc = _drop(dim, solid_model)
            data = _run(sc)
        got, digest = data.read_particles(), _digest(data)
        st = data.stats()
        assert st["overflow"] == 0
        assert np.array_equal(data.read_particle_models(), sc["models"]), names
        if ref is None:
            ref = (got, digest)
            again = _run(_drop(dim, solid_model))
            assert _digest(again) == digest
            _assert_same_particles(again.read_particles(), got, "two runs")
            assert all(np.isfinite(getattr(got, f)).all() for f in ("pos", "vel", "def_grad", "affine"))
            assert st["cell_changers"] > 0, "stir the scene: nobody changed cell"
            # every collider is felt by at least one face layer of the tank's lattice (the smallest face: 12 x 16 in 3D, 24 in 2D; the
            # first layer stands 0.45 - 0.55 cells off its collider)
            layer = 12 * 16 if dim == 3 else 24
            for c in range(len(sc["colliders"])):
                assert ((got.cdf_affinity >> c) & 1).sum() >= layer, f"collider {c}: the tank should feel its floor and walls"
            solid = sc["models"] != MODEL_FLUID
            eye = np.eye(dim, dtype=np.float32).reshape(-1)
            assert np.array_equal(got.def_grad[~solid][:, 1:], np.tile(eye[1:], (int((~solid).sum()), 1)))
            assert np.abs(got.def_grad[solid] - eye).max() > 1e-3, "the block should feel the fluid"
            continue
        assert_same_bits(got, ref[0], FIELDS, names)
        assert digest == ref[1], names


@pytest.mark.parametrize("dim,solid_model", [(3, MODEL_COROTATED), (2, MODEL_NEO_HOOKEAN)])
def test_restart_continues_bit_for_bit(hip_libs, dim, solid_model):
    """10 substeps -> read_particles + read_particle_models -> new data + the table -> 10 substeps == 20 substeps, fields and digest."""
    sc = _drop(dim, solid_model)
    whole = _run(sc, (10, 10))
    first = _run(sc, (10,))
    snap, labels = first.read_particles(), first.read_particle_models()
    assert np.array_equal(labels, sc["models"])
    rest = _run(dict(sc, particles=snap, models=labels), (10,))
    assert_same_bits(whole.read_particles(), rest.read_particles(), BASE_FIELDS)
    assert _digest(whole) == _digest(rest)
    assert np.array_equal(rest.read_particle_models(), sc["models"])


# ------------------------------------------------------------------------------------------------ 6. diagnostics and drawing
@pytest.mark.parametrize("dim,solid_model", [(3, MODEL_COROTATED), (3, MODEL_NEO_HOOKEAN), (2, MODEL_COROTATED), (2, MODEL_NEO_HOOKEAN)])
def test_diagnostics_and_vertex_buffer_go_by_the_particles_model(hip_libs, dim, solid_model):
    sc, _, _ = mt.coupled_truths(dim, solid_model, "random")
    fl = sc["fluid"]
    gamma = sc["fluid_gamma"]
    _, data = new_data(sc, models=None)
    before = data.diagnostics(_ffi.DIAG_PARTICLES)
    data.set_particle_models(sc["models"])
    after = data.diagnostics(_ffi.DIAG_PARTICLES)
    assert before.model == solid_model and after.model == MODEL_PER_PARTICLE
    for name in ("mass", "momentum"):                                   # the table does not touch them
        assert np.array_equal(before.sums[name].fixed, after.sums[name].fixed) and before.sums[name].exponent == after.sums[name].exponent
    data.pipeline.step(data, 20)
    data.sync()
    d = data.diagnostics(_ffi.DIAG_ALL)
    got = data.read_particles()
    assert d.model == MODEL_PER_PARTICLE and d.num_particles == got.n and d.num_nonfinite == 0
    vol = got.init_volume.astype(np.float64)
    pf = ft.psi_parts(got.def_grad[fl][:, 0], got.lambda_[fl], gamma) * vol[fl][:, None]
    pso = dt_.psi_parts(solid_model, dt_._mat(got.def_grad[~fl], dim), got.lambda_[~fl], got.mu[~fl]) * vol[~fl][:, None]
    truth = math.fsum(pf.sum(1)) + math.fsum(pso.sum(1))
    s = d.sums["elastic"]
    bound = got.n * 2.0 ** (s.exponent - 1) + 2 * ELASTIC_ROUNDINGS * U * (math.fsum(np.abs(pf).sum(1)) + math.fsum(np.abs(pso).sum(1)))
    err = abs(float(s.value[0]) - truth)
    report_margin(f"mixed {dim}D solid={solid_model} elastic |value - truth|", err, bound, exponent=s.exponent)
    assert truth > 0.0 and err <= bound, (err, bound, truth)
    # under ONE model the sum is another one: the table is what the diagnostics went by
    one = math.fsum((dt_.psi_parts(solid_model, dt_._mat(got.def_grad, dim), got.lambda_, got.mu) * vol[:, None]).sum(1))
    assert abs(one - truth) > 100 * bound
    # drawing: cbrt(J) I / sqrt(J) I for the fluid rows, F for the others
    inst = data.prep_vertex_buffer(0)
    ref = np_oracle.prep_instances(got.pos, got.vel, got.def_grad, got.cdf_normal, got.cdf_dist, got.cdf_affinity, 0, sc["cell_width"],
                                   sc["params"].dt, np.ones((got.n, 4), np.float32))
    assert np.array_equal(inst[~fl][:, :20], ref[~fl][:, :20].astype(np.float32))
    J = got.def_grad[fl][:, 0].astype(np.float64)
    iso = np.cbrt(J) if dim == 3 else np.sqrt(J)
    for c in range(3):
        col = inst[fl][:, 4 * c:4 * c + 3]
        assert np.allclose(col[:, c], iso if c < dim else 1.0, rtol=3e-7, atol=0)
        assert np.all(np.delete(col, c, axis=1) == 0.0)
    assert np.array_equal(inst[fl][:, 12:20], ref[fl][:, 12:20].astype(np.float32))


# ------------------------------------------------------------------------------------------------ 7. arguments
@pytest.mark.parametrize("dim", [3, 2])
def test_refusals_leave_the_data_alone(hip_libs, dim):
    sc, _, _ = mt.coupled_truths(dim, MODEL_NEO_HOOKEAN, "plane")
    _, data = new_data(sc)
    data.pipeline.step(data, 3)
    data.sync()
    state = (_digest(data), data.read_particles(), data.read_particle_models())

    def unchanged(d, st):
        assert _digest(d) == st[0]
        _assert_same_particles(d.read_particles(), st[1])
        assert np.array_equal(d.read_particle_models(), st[2])
    # an entry that is no model
    bad = sc["models"].copy()
    bad[-1] = 3
    with pytest.raises(WgsError) as e:
        data.set_particle_models(bad)
    assert e.value.code == _ffi.ERR_INVALID_ARGUMENT and "entry" in str(e.value)              # through wgs_last_error
    unchanged(data, state)
    with pytest.raises(WgsError) as e:
        data.set_constitutive_model(MODEL_PER_PARTICLE)                 # never a model to select
    assert e.value.code == _ffi.ERR_INVALID_ARGUMENT
    unchanged(data, state)
    # the same table again: not a bit changes
    data.set_particle_models(sc["models"])
    unchanged(data, state)
    assert data.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_PER_PARTICLE
    # NULL drops the table: the data's single model again, F as it is; device memory is given back
    bytes_with = data.stats()["device_bytes"]
    data.set_particle_models(None)
    assert data.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_NEO_HOOKEAN
    assert np.all(data.read_particle_models() == MODEL_NEO_HOOKEAN)
    assert _digest(data) == state[0]
    assert 0 < bytes_with - data.stats()["device_bytes"] <= 2 * (sc["particles"].n + 64)
    # set_constitutive_model after a table: that model, no table
    data.set_particle_models(sc["models"])
    data.set_constitutive_model(MODEL_COROTATED)
    assert data.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_COROTATED
    assert np.all(data.read_particle_models() == MODEL_COROTATED)
    data.pipeline.step(data, 2)
    data.sync()
    assert data.stats()["overflow"] == 0

    # data whose step carries plastic state
    ps = scenes.random_cloud(800, dim=dim, seed=3, young=1e6, plasticity=DruckerPrager.new(1e6, 0.25), phase=None)
    _, pl = new_data(dict(particles=ps, params=SimulationParams((0.0, -9.81, 0.0)[:dim], 8e-4), colliders=[], cell_width=1.0, grid_capacity=4096,
                          model=MODEL_NEO_HOOKEAN))
    pl.pipeline.step(pl, 2)
    pl.sync()
    st = (_digest(pl), pl.read_particles(), pl.read_particle_models())
    assert np.all(st[2] == MODEL_NEO_HOOKEAN)
    with pytest.raises(WgsError) as e:
        pl.set_particle_models(np.zeros(ps.n, np.uint8))
    assert e.value.code == _ffi.ERR_UNSUPPORTED and "plastic" in str(e.value)
    unchanged(pl, st)
    assert pl.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_NEO_HOOKEAN
    pl.set_particle_models(None)                                        # nothing to drop: fine


def test_sharded_data_is_refused(hip_libs):
    sc = scenes.tait_fluid_block(32, 16, 16, with_floor=False)
    pipe = pipeline(3)
    shards, _ = lockstep_slabs(pipe, sc, 2)
    s = shards[0]
    before = s.diagnostics(_ffi.DIAG_DIGEST).digest
    table = np.zeros(sc["particles"].n, np.uint8)
    for arg in (table.ctypes.data_as(C.POINTER(C.c_uint8)), None):
        assert s.lib.wgs_set_particle_models(s._h, arg) == _ffi.ERR_UNSUPPORTED
        assert b"sharded" in s.lib.wgs_last_error()
    assert s.lib.wgs_read_particle_models(s._h, table.ctypes.data_as(C.POINTER(C.c_uint8))) == _ffi.ERR_UNSUPPORTED
    assert s.diagnostics(_ffi.DIAG_DIGEST).digest == before
    assert s.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_FLUID
