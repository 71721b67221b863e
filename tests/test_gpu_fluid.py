"""-m gpu: the weakly-compressible fluid model (MODEL_FLUID) on the device: parity with the fp64 truth of tests/fluid_truth.py,
bit identity across launch shapes, checkpoint / model switches, diagnostics, argument checks, sharded data.

Figures measured on one MI355X are in profiles/r09_fluid_margins.json (every comparison goes through helpers.report_margin)."""
import contextlib
import math

import numpy as np
import pytest

import fluid_truth as ft
from gpu_common import GRID_V_TOL, PART_TOL
from helpers import BASE_FIELDS, assert_close_to_truth, assert_joined_close, assert_same_bits, debug, new_data, pipeline, report_margin
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd._ffi import WgsError
from wgsparkl_amd.models import MODEL_FLUID, MODEL_NEO_HOOKEAN, DruckerPrager, FluidCoefficients, ParticlePhase
from wgsparkl_amd.sharded import join_slabs, lockstep_slabs
from wgsparkl_amd.solver import ParticleSet, SimulationParams

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ELASTIC_ROUNDINGS = 256    # the allowance tests/test_gpu_diagnostics.py gives the elastic sum of the other models


def _run(sc, calls=(12, 12)):
    _, data = new_data(sc)
    for k in calls:
        data.pipeline.step(data, k)
    data.sync()
    return data


def _falling_block(dim, uniform, visc, gamma, seed=4):
    """A jittered block in free fall whose initial velocity field compresses and shears it."""
    h = 1.0
    counts = (16, 16, 16) if dim == 3 else (40, 40)
    pos = scenes.lattice(counts, (9.0,) * dim, h, 0.05, seed=seed)
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, FluidCoefficients(2.0e5, visc), phase=ParticlePhase(1.0, scenes.FLT_MAX))   # (no plastic state)
    c = pos.mean(0)
    ps.vel[:] = ((c - pos) * 2.5).astype(np.float32)                   # converging: J falls by some 10 % over the run
    ps.vel[:, 0] += ((pos[:, 1] - c[1]) * 3.0).astype(np.float32)      # shear
    if not uniform:
        rng = np.random.default_rng(seed + 1)
        ps.lambda_[:] = (ps.lambda_ * rng.uniform(0.7, 1.3, ps.n)).astype(np.float32)
        ps.mu[:] = (ps.mu * rng.uniform(0.5, 1.5, ps.n)).astype(np.float32)
        ps.mass[:] = (ps.mass * rng.uniform(0.8, 1.2, ps.n)).astype(np.float32)
    return dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0), colliders=[], cell_width=h,
                grid_capacity=4096, model=MODEL_FLUID, fluid_gamma=gamma)


def _assert_canonical(got, dim):
    """def_grad of a fluid particle is diag(J, 1[, 1]) exactly."""
    eye = np.eye(dim, dtype=np.float32).reshape(-1)
    assert np.array_equal(got.def_grad[:, 1:], np.tile(eye[1:], (got.n, 1)))


@pytest.mark.parametrize("visc,gamma", [(0.0, 7.0), (30.0, 4.0)])
@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("dim", [3, 2])
def test_parity_with_the_fp64_truth(hip_libs, dim, uniform, visc, gamma):
    """24 substeps over two calls: blocks and cells exact by virtual id; grid velocity, position, velocity, J within the bounds of the
    elastic scenes (1e-5 grid, 2e-5 particle); `affine` — which carries the gamma-fold amplified rounding of J — through
    assert_close_to_truth with the fp32 run of the truth as ref32."""
    sc = _falling_block(dim, uniform, visc, gamma)
    ps = sc["particles"]
    data = _run(sc, (12, 12))
    st64 = ft.FluidState(ps, sc["params"], 1.0, gamma, np.float64)
    st32 = ft.FluidState(ps, sc["params"], 1.0, gamma, np.float32)
    st64.step(24)
    st32.step(24)
    tag = f"fluid {dim}D {'uniform' if uniform else 'mixed'} mu={visc:g} gamma={gamma:g}"
    assert st64.J.min() < 0.95, "the scene should compress"
    # blocks
    vid, first, num, ids = data.read_blocks()
    tv, tn = st64.active_blocks()
    assert np.array_equal(vid, tv), "active block sets differ"
    assert np.array_equal(num, tn), "per-block particle counts differ"
    assert sorted(ids.tolist()) == list(range(ps.n))
    # grid
    cells, vm = data.read_grid()[:2]
    tc, tvm = st64.grid_records()
    assert np.array_equal(cells, tc), "active node cells differ"
    v32, m32 = st32.grid_at(tc.astype(np.int64))
    assert_close_to_truth(f"{tag}: grid velocity", vm[:, :dim], v32, tvm[:, :dim], GRID_V_TOL)
    assert_close_to_truth(f"{tag}: grid mass", vm[:, dim], m32, tvm[:, dim], GRID_V_TOL)
    # particles
    got = data.read_particles()
    _assert_canonical(got, dim)
    assert_close_to_truth(f"{tag}: pos", got.pos, st32.pos, st64.pos, PART_TOL)
    assert_close_to_truth(f"{tag}: vel", got.vel, st32.vel, st64.vel, PART_TOL)
    assert_close_to_truth(f"{tag}: J", got.def_grad[:, 0], st32.J, st64.J, PART_TOL)
    assert_close_to_truth(f"affine ({tag})", got.affine, st32.C, st64.C, PART_TOL)
    assert np.array_equal(got.lambda_, ps.lambda_) and np.array_equal(got.mu, ps.mu) and np.array_equal(got.mass, ps.mass)
    assert data.stats()["overflow"] == 0


def _state(data):
    got = data.read_particles()
    return got, data.diagnostics(_ffi.DIAG_DIGEST).digest


FIELDS = ("pos", "vel", "def_grad", "affine", "cdf_affinity", "cdf_dist")
SHAPES = ((), ("G2P_TWO_PASSES",), ("G2P_TWO_LAUNCHES",), ("REBIN_LAUNCH",), ("NO_UNIFORM",))


@pytest.mark.parametrize("scene", ["block3", "block2", "dam_break"])
def test_launch_shapes_and_runs_are_bit_identical(hip_libs, monkeypatch, scene):
    """The default run twice, and under each launch-shape switch: the same bits. The dam break stands against a floor and a wall, so the
    near-collider list walk and the CPIC paths advance fluid particles; nothing may end up behind a collider deeper than the elastic
    scenes' tests allow (half a cell), nothing may be non-finite, the grid may not overflow."""
    def make():
        if scene == "dam_break":
            return scenes.dam_break(viscosity=5.0)
        return _falling_block(3 if scene == "block3" else 2, True, 10.0, 7.0)
    ref = None
    for names in SHAPES:
        with debug(monkeypatch, *names) if names else contextlib.nullcontext():
            data = _run(make(), (15, 15))
        got, digest = _state(data)
        assert data.stats()["overflow"] == 0
        if ref is None:
            ref = (got, digest)
            got2, digest2 = _state(_run(make(), (15, 15)))             # two runs
            assert digest2 == digest
            assert_same_bits(got2, got, FIELDS)
            assert np.isfinite(got.pos).all() and np.isfinite(got.vel).all() and np.isfinite(got.def_grad).all() and np.isfinite(got.affine).all()
            _assert_canonical(got, got.dim)
            if scene == "dam_break":
                assert (got.cdf_affinity != 0).sum() > 500, "the column should feel the floor and the wall"
                assert got.pos[:, 1].min() > 2.0 - 0.5 and got.pos[:, 0].min() > 8.0 - 0.5
                assert np.abs(got.def_grad[:, 0] - 1.0).max() > 1e-4
            continue
        assert_same_bits(got, ref[0], FIELDS, names)
        assert digest == ref[1], names


@pytest.mark.parametrize("dim", [3, 2])
def test_checkpoint_and_model_switches(hip_libs, dim):
    """Read back after k substeps, recreate, select the fluid, continue: the digest of the uninterrupted run. Switching 1 -> 2 -> 1
    mid-run leaves a state the neo-Hookean step accepts, reproducibly."""
    sc = _falling_block(dim, True, 10.0, 5.0)
    whole = _run(sc, (10, 14))
    first = _run(sc, (10,))
    mid = first.read_particles()
    _assert_canonical(mid, dim)
    sc2 = dict(sc, particles=mid)
    rest = _run(sc2, (14,))
    assert_same_bits(whole.read_particles(), rest.read_particles(), BASE_FIELDS)
    assert whole.diagnostics(_ffi.DIAG_DIGEST).digest == rest.diagnostics(_ffi.DIAG_DIGEST).digest
    # selecting the fluid again changes nothing
    before = rest.diagnostics(_ffi.DIAG_DIGEST).digest
    rest.set_constitutive_model(MODEL_FLUID)
    assert rest.diagnostics(_ffi.DIAG_DIGEST).digest == before

    def switched():
        s = _falling_block(dim, True, 0.0, 7.0)
        s["model"] = MODEL_NEO_HOOKEAN
        _, d = new_data(s)
        d.pipeline.step(d, 8)
        pre = d.read_particles()
        d.set_constitutive_model(MODEL_FLUID)
        col = d.read_particles()
        d.pipeline.step(d, 8)
        d.set_constitutive_model(MODEL_NEO_HOOKEAN)
        d.pipeline.step(d, 8)
        d.sync()
        return pre, col, d.read_particles(), d.diagnostics(_ffi.DIAG_DIGEST)
    pre, col, end, dg = switched()
    _assert_canonical(col, dim)
    det = np.linalg.det(ft._mat(pre.def_grad.astype(np.float64), dim))
    assert np.max(np.abs(col.def_grad[:, 0] - det)) <= 8 * np.spacing(np.float32(1.0)) * np.max(np.abs(pre.def_grad)) ** dim   # (an fp32 determinant: under 8 roundings of products of that size)
    assert np.isfinite(end.pos).all() and np.isfinite(end.affine).all() and np.isfinite(end.def_grad).all()
    assert np.abs(end.def_grad[:, 1:] - col.def_grad[:, 1:]).max() > 0, "the neo-Hookean step should have sheared F again"
    assert dg.model == MODEL_NEO_HOOKEAN
    assert switched()[3].digest == dg.digest


@pytest.mark.parametrize("dim,gamma", [(3, 7.0), (2, 4.0)])
def test_elastic_sum_and_model_in_the_diagnostics(hip_libs, dim, gamma):
    """WGS_SUM_ELASTIC = sum V0 Psi(Jc) against the fp64 truth of the read-back, by the rule of tests/test_gpu_diagnostics.py:
    |value - truth| <= N 2^(exponent-1) + 2 x roundings x 2^-53 x sum |pieces|."""
    sc = _falling_block(dim, False, 10.0, gamma)
    data = _run(sc, (20,))
    d = data.diagnostics(_ffi.DIAG_ALL)
    got = data.read_particles()
    assert d.model == MODEL_FLUID and d.num_particles == got.n and d.num_nonfinite == 0
    parts = ft.psi_parts(got.def_grad[:, 0], got.lambda_, gamma) * got.init_volume.astype(np.float64)[:, None]
    truth = math.fsum(parts.sum(1))
    s = d.sums["elastic"]
    bound = got.n * 2.0 ** (s.exponent - 1) + 2 * ELASTIC_ROUNDINGS * U * math.fsum(np.abs(parts).sum(1))
    err = abs(float(s.value[0]) - truth)
    report_margin(f"fluid {dim}D elastic |value - truth|", err, bound, exponent=s.exponent)
    assert truth > 0.0 and err <= bound, (err, bound, truth)
    assert s.value[0] == math.ldexp(int(s.fixed[0]), s.exponent)
    assert abs(d.min_det_f - float(got.def_grad[:, 0].min())) <= 2 * float(np.spacing(np.float32(1.0)))


@pytest.mark.parametrize("dim", [3, 2])
def test_unsupported_on_plastic_data_and_eos_argument_checks(hip_libs, dim):
    ps = scenes.random_cloud(800, dim=dim, seed=3, young=1e6, plasticity=DruckerPrager.new(1e6, 0.25), phase=None)
    sc = dict(particles=ps, params=SimulationParams((0.0, -9.81, 0.0)[:dim], 8e-4), colliders=[], cell_width=1.0, grid_capacity=4096,
              model=MODEL_NEO_HOOKEAN)
    _, data = new_data(sc)
    with pytest.raises(WgsError) as e:
        data.set_constitutive_model(MODEL_FLUID)
    assert e.value.code == _ffi.ERR_UNSUPPORTED
    assert data.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_NEO_HOOKEAN
    data.pipeline.step(data, 2)
    data.sync()
    for bad in (1.0, 0.5, -7.0, float("nan"), float("inf")):
        with pytest.raises(WgsError) as e:
            data.set_fluid_eos(bad)
        assert e.value.code == _ffi.ERR_INVALID_ARGUMENT
    data.set_fluid_eos(1.5)                                             # allowed under any model
    with pytest.raises(WgsError) as e:
        data.set_constitutive_model(3)
    assert e.value.code == _ffi.ERR_INVALID_ARGUMENT


def test_gamma_is_read_by_the_fluid_only_and_matters(hip_libs):
    sc = _falling_block(3, True, 0.0, 7.0)
    a = _run(sc, (10,)).read_particles()
    b = _run(dict(sc, fluid_gamma=3.0), (10,)).read_particles()
    assert not np.array_equal(a.affine, b.affine)
    nh = dict(sc, model=MODEL_NEO_HOOKEAN)
    c = _run(nh, (10,)).read_particles()
    e = _run(dict(nh, fluid_gamma=3.0), (10,)).read_particles()
    assert np.array_equal(c.affine, e.affine) and np.array_equal(c.def_grad, e.def_grad)


def test_vertex_buffer_draws_the_isotropic_deformation(hip_libs):
    sc = _falling_block(3, True, 0.0, 7.0)
    data = _run(sc, (10,))
    got = data.read_particles()
    inst = data.prep_vertex_buffer(0)
    s = np.cbrt(got.def_grad[:, 0].astype(np.float64))
    for c in range(3):
        col = inst[:, 4 * c:4 * c + 3]
        assert np.allclose(col[:, c], s, rtol=3e-7, atol=0)
        assert np.all(np.delete(col, c, axis=1) == 0.0)


@pytest.mark.parametrize("world", [2, 3])
def test_fluid_block_as_lockstep_slabs_matches_the_single_domain(hip_libs, world, monkeypatch):
    """The comparison and the bounds tests/test_gpu_sharded.py applies to its elastic bar (80 substeps over two calls, a table rebuild
    inside, particles migrate): 1e-5 on position, velocity, def_grad, 2e-4 on affine."""
    from wgsparkl_amd.sharded import native_lockstep
    monkeypatch.setenv("WGS_REHASH_PERIOD", "64")
    sc = scenes.tait_fluid_block(24 * world, 24, 24, with_floor=False, viscosity=20.0, gamma=7.0)
    ps = sc["particles"]
    rng = np.random.default_rng(8)
    ps.vel[:] = rng.normal(0.0, 3.0, ps.vel.shape).astype(np.float32)
    ps.vel[:, 0] += 8.0
    k = 80
    ref = _run(sc, (k,)).read_particles()
    pipe = pipeline(3)
    shards, part = lockstep_slabs(pipe, sc, world)
    assert part.min_interior_width() >= 3
    n0 = [s.num_particles() for s in shards]
    native_lockstep(pipe, shards, 30)
    native_lockstep(pipe, shards, k - 30)
    for s in shards:
        s.sync()
    joined = join_slabs([s.export() for s in shards], np.arange(ps.n))
    assert joined.exact, joined.problem
    assert joined.counts != n0, "the test scene must make particles migrate"
    assert np.abs(ref.def_grad[:, 0] - 1.0).max() > 1e-3
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 1e-5), ("def_grad", 1e-5), ("affine", 2e-4)), f"fluid, {world} lockstep slabs, {{f}}")
