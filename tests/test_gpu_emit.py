"""-m gpu: particles added at run time (include/wgsparkl_hip_emit.h). The truth needs no tolerance: tests/test_gpu_bit_identity.py
establishes checkpoint -> restart as bit-exact, so data that had particles added must end bit for bit where a twin ends that was created
from the same union in the same order. Emitters are held to the append path: a twin without emitters gets the batches of
tests/emit_truth.py by hand, in front of the scheduled substeps."""
import ctypes as C
import contextlib
from fractions import Fraction

import numpy as np
import pytest

import emit_truth as ET
from helpers import CDF_FIELDS, _digest, debug, new_data, restored_colliders
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd.models import (MODEL_COROTATED, MODEL_FLUID, DruckerPrager, ElasticCoefficients, Emitter, FluidCoefficients, ForceField,
                                 ParticlePhase)
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider, ParticleSet, SimulationParams

pytestmark = pytest.mark.gpu
FLT_MAX = float(np.finfo(np.float32).max)
EVERY_FIELD = CDF_FIELDS + ("phase", "dp", "mass", "lambda_", "mu", "init_volume", "init_radius", "cdf_rigid_vel", "has_plasticity", "has_phase")


def assert_same_bits(a, b, fields, tag=None):
    """The same BITS field by field (helpers.assert_same_bits compares values: a NaN equals nothing there, and a particle in the corner of
    three colliders can carry a NaN cdf normal in every run alike): fp32 fields are compared as their uint32 words."""
    for f in fields:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        if x.dtype == np.float32 and y.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert x.shape == y.shape and np.array_equal(x, y), f if tag is None else (tag, f)


def sub(ps, sel):
    return ParticleSet(**{k: (v[sel].copy() if isinstance(v, np.ndarray) else v) for k, v in ps.__dict__.items()})


def cat(*sets):
    return ParticleSet(**{k: (np.concatenate([getattr(s, k) for s in sets]) if isinstance(v, np.ndarray) else v) for k, v in sets[0].__dict__.items()})


def split(ps, n1):
    return sub(ps, slice(0, n1)), sub(ps, slice(n1, None))


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


def added_and_twin(sc, n1, steps_before=0, **kw):
    """(data created with the first n1 particles of the scene and room for all, the rest, the scene's models split alike)"""
    full = sc["particles"]
    p1, p2 = split(full, n1)
    m = sc.get("models")
    over = dict(particles=p1, particle_capacity=full.n, **kw)
    if m is not None:
        over["models"] = m[:n1]
    pipe, data = new_data(sc, **over)
    return pipe, data, p1, p2, (m[n1:] if m is not None else None)


# ------------------------------------------------------------------------------------------------ 1. added at substep 0 == created together
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
    """def_grad off the identity, so that diag(det F, 1[, 1]) of a fluid particle is not the identity it started from"""
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
        perm = np.random.default_rng(8).permutation(sc["particles"].n)        # fluid and solid labels on both sides of the split
        return {**sc, "particles": sub(sc["particles"], perm), "models": sc["models"][perm]}
    raise KeyError(name)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["general", "uniform", "dp2", "dp1", "dp0", "fluid", "table"])
def test_added_at_substep_0_equals_created_together(hip_libs, name, dim):
    sc = _case(name, dim)
    n = sc["particles"].n
    n1 = (2 * n) // 3 + 1
    pipe, data, p1, p2, m2 = added_and_twin(sc, n1)
    assert data.particle_capacity == n and data.n == n1
    data.add_particles(p2, models=m2)
    assert data.n == n and data.stats()["num_particles"] == n
    _, twin = new_data(sc)
    assert_same_state(data, twin, (name, dim, "before any substep"), models=True)
    if m2 is not None:
        assert (m2 == MODEL_FLUID).any() and (m2 != MODEL_FLUID).any()
    for d in (data, twin):
        pipe.step(d, 12)
        d.sync()
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
def test_added_mid_run_equals_a_restart_from_the_union(hip_libs, monkeypatch, tag, sc, switches):
    """Step 7, add, step 13 against: the snapshot after 7 substeps U the added particles, created anew with its plastic state and restored
    colliders, stepped 13."""
    with debug(monkeypatch, *switches) if switches else contextlib.nullcontext():
        n = sc["particles"].n
        pipe, data, p1, p2, _ = added_and_twin(sc, (3 * n) // 4)
        data.set_plastic_state(p1.dp_state)
        pipe.step(data, 7)
        data.sync()
        snap, bodies = data.read_particles(), data.read_body_poses()
        rebuilds = data.stats()["table_rebuilds"]
        data.add_particles(p2)
        union = cat(snap, p2)
        _, twin = new_data(sc, particles=union, colliders=restored_colliders(sc["colliders"], bodies, 3))
        twin.set_plastic_state(union.dp_state)
        assert_same_bits(data.read_particles(), union, ("pos", "vel", "def_grad", "affine", "dp_state", "mass"), (tag, "read between the add and the step"))
        pipe.step(data, 13)
        pipe.step(twin, 13)
        data.sync()
        twin.sync()
        assert data.stats()["table_rebuilds"] == rebuilds + 1, "the substep after the add rebuilds the table, and no other"
        assert_same_state(data, twin, tag)
        assert data.diagnostics().num_nonfinite == 0 and data.stats()["substeps_done"] == 20


# ------------------------------------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_small_batches_around_a_wave(hip_libs, k):
    ps = cloud(3, 700 + k, seed=40 + k)
    sc = scene_of(ps)
    pipe, data, p1, p2, _ = added_and_twin(sc, 700)
    pipe.step(data, 2)
    data.add_particles(p2)
    snap = sub(data.read_particles(), slice(0, 700))
    _, twin = new_data(sc, particles=cat(snap, p2))
    for d in (data, twin):
        pipe.step(d, 3)
        d.sync()
    assert_same_state(data, twin, k)


def test_capacity_is_filled_exactly_and_one_more_is_refused_without_a_trace(hip_libs):
    ps = cloud(3, 900, seed=50)
    sc = scene_of(ps)
    pipe, data, p1, p2, _ = added_and_twin(sc, 600)
    pipe.step(data, 3)
    data.sync()
    a, b = split(p2, 100)
    data.add_particles(a)                       # two adds without a step between them
    data.add_particles(b)
    assert data.n == data.particle_capacity == 900
    before, stats = _digest(data), data.stats()
    with pytest.raises(_ffi.WgsError) as err:
        data.add_particles(sub(p2, slice(0, 1)))
    assert err.value.code == _ffi.ERR_INVALID_ARGUMENT and "capacity is 900" in str(err.value)
    assert _digest(data) == before and data.n == 900 and data.stats() == stats
    snap = sub(data.read_particles(), slice(0, 600))
    _, twin = new_data(sc, particles=cat(snap, a, b))
    for d in (data, twin):
        pipe.step(d, 5)
        d.sync()
    assert_same_state(data, twin, "full")
    # data created without a reservation has room for nothing
    _, plain = new_data(sc)
    assert plain.particle_capacity == 900
    with pytest.raises(_ffi.WgsError):
        plain.add_particles(a)


def test_into_a_full_block_far_away_and_into_empty_data(hip_libs):
    dense = block(3, (8, 8, 8), origin=(8.0, 8.0, 8.0))                      # one block (cells 8..11), 512 residents
    inside = block(3, (6, 6, 6), origin=(8.3, 8.3, 8.3), seed=9)              # ... and 216 more into it
    far = block(3, (4, 4, 4), origin=(8.0 + 80.0, 8.0, 8.0), seed=10)         # twenty blocks of four cells along x away
    sc = scene_of(cat(dense, inside, far))
    pipe, data = new_data(sc, particles=dense, particle_capacity=sc["particles"].n)
    pipe.step(data, 4)
    data.sync()
    assert data.stats()["num_active_blocks"] <= 27
    snap = data.read_particles()
    data.add_particles(inside)
    data.add_particles(far)
    _, twin = new_data(sc, particles=cat(snap, inside, far))
    for d in (data, twin):
        pipe.step(d, 6)
        d.sync()
    assert_same_state(data, twin, "dense block and far block")
    # data created EMPTY: the general layouts, no plastic state; everything it holds was added
    both = cloud(3, 800, seed=61)
    sc = scene_of(both, [floor(3)])
    pipe, empty = new_data(sc, particles=sub(both, slice(0, 0)), particle_capacity=800)
    assert empty.n == 0 and empty.particle_capacity == 800 and empty.read_positions().shape == (0, 3)
    pipe.step(empty, 2)                                                       # (substeps of nothing)
    empty.add_particles(both)
    _, twin = new_data(sc)
    assert_same_bits(empty.read_particles(), both, ("pos", "vel", "def_grad", "affine", "mass", "lambda_", "mu"), "empty, read")
    for d in (empty, twin):
        pipe.step(d, 6)
        d.sync()
    assert_same_bits(empty.read_particles(), twin.read_particles(), EVERY_FIELD, "created empty")


def test_readers_between_the_add_and_the_step_and_the_mass_sum(hip_libs):
    sc = _case("table", 3, perturb=False)         # (F = 1: det F is 1 whatever the rounding)
    n = sc["particles"].n
    pipe, data, p1, p2, m2 = added_and_twin(sc, n // 2)
    pipe.step(data, 5)
    data.sync()
    snap, models = data.read_particles(), data.read_particle_models()
    mass0 = data.diagnostics().sums["mass"]
    data.add_particles(p2, models=m2)
    got = data.read_particles()
    assert got.n == n
    assert_same_bits(sub(got, slice(0, n // 2)), snap, EVERY_FIELD, "the residents")
    want = p2.copy()
    fl = m2 == MODEL_FLUID                      # def_grad of a fluid label: diag(det F, 1, 1)
    want.def_grad[fl] = np.eye(3, dtype=np.float32).reshape(-1)
    assert_same_bits(sub(got, slice(n // 2, None)), want, ("pos", "vel", "def_grad", "affine", "mass", "lambda_", "mu", "init_volume", "init_radius", "phase"), "the new ones")
    # (no particle of the scene has plasticity: the parameters read back are the library's defaults, the ones creation gave the residents)
    assert np.array_equal(got.dp[n // 2:].view(np.uint32), np.tile(snap.dp[:1].view(np.uint32), (n - n // 2, 1))) and not got.has_plasticity.any()
    assert np.array_equal(data.read_positions(), np.concatenate([snap.pos, p2.pos]))
    assert np.array_equal(data.read_particle_models(), np.concatenate([models, m2]))
    assert data.prep_vertex_buffer().shape == (n, 24) and np.array_equal(data.prep_vertex_buffer()[:, 12:15], np.concatenate([snap.pos, p2.pos]))
    assert data.particle_fields().model.shape == (n,) and data.diagnostics().num_particles == n
    mass1 = data.diagnostics().sums["mass"]
    exact = lambda s: Fraction(int(s.fixed[0])) * Fraction(2) ** int(s.exponent)
    assert exact(mass1) - exact(mass0) == sum(Fraction(float(m)) for m in p2.mass), "WGS_SUM_MASS grows by exactly the added masses"


# ------------------------------------------------------------------------------------------------ 4. emitters against the append path
def _two_emitters(dim, base):
    proto = sub(base, slice(3, 4))
    proto.vel[0] = (0.3, -2.0, 0.1)[:dim]
    proto2 = sub(base, slice(8, 9))
    proto2.vel[0] = (-0.5, -1.0, 0.4)[:dim]
    return [Emitter(proto, (3.0, 9.5, 3.0)[:dim], (3, 2, 3)[:dim], 0.5, jitter=0.3, seed=11, start_substep=1, period=3),
            Emitter(proto2, (6.0, 8.0, 5.0)[:dim], (2, 2, 2)[:dim], 0.45, jitter=0.0, seed=5, start_substep=0, period=5, batches=4)]


@pytest.mark.parametrize("dim,timestamps", [(3, False), (2, False), (3, True)])
def test_emitters_equal_the_append_path(hip_libs, dim, timestamps):
    base = cloud(dim, 900, seed=70 + dim)
    ems = _two_emitters(dim, base)
    events, emitted, skipped, n_end = ET.run_schedule(ems, base.n, 10 ** 6, 24)
    sc = scene_of(base, [floor(dim)])
    pipe, data = new_data(sc, particle_capacity=n_end, emitters=ems)
    assert [(e.lo, e.count, e.period, e.start_substep, e.batches, e.seed) for e in data.emitters()] == [(e.lo, e.count, e.period, e.start_substep, e.batches, e.seed) for e in ems]
    for k in (1, 5, 18):
        pipe.step(data, k, timestamps)
        data.sync()
    _, twin = new_data(sc, particle_capacity=n_end)
    for s in range(24):
        for s_e, e, q in events:
            if s_e == s:
                twin.add_particles(ET.batch_particles(ems[e], e, q))
        pipe.step(twin, 1)
    twin.sync()
    assert data.n == twin.n == n_end == data.stats()["num_particles"]
    assert data.emitter_counts() == (emitted, skipped) and skipped == [0, 0]
    assert ET.scheduled_batches(ems[0], 24) * ems[0].batch_size == emitted[0] and emitted[1] == 4 * ems[1].batch_size
    assert_same_state(data, twin, ("emitters", dim, timestamps))
    assert data.stats()["table_rebuilds"] == twin.stats()["table_rebuilds"] == 1 + len({s for s, _, _ in events if s > 0})
    if timestamps:
        assert data.read_timings()["grid sort"] > 0.0


def test_a_batch_that_does_not_fit_is_skipped_and_counted(hip_libs):
    base = cloud(3, 500, seed=81)
    proto = sub(base, slice(0, 1))
    em = Emitter(proto, (4.0, 9.0, 4.0), (5, 2, 1), 0.5, period=2)           # 10 per batch at substeps 0, 2, 4, ..
    pipe, data = new_data(scene_of(base), particle_capacity=525, emitters=[em])
    pipe.step(data, 9)
    data.sync()                                                              # (no error bit: wgs_sync succeeds)
    st = data.stats()
    assert data.emitter_counts() == ([20], [3]) and data.n == st["num_particles"] == 520 and st["overflow"] == 0
    assert ET.run_schedule([em], 500, 525, 9)[1:] == ([20], [3], 520)
    assert data.diagnostics().num_nonfinite == 0 and data.read_particles().n == 520
    pipe.step(data, 4)                                                       # the run goes on
    data.sync()
    assert data.n == 520 and data.emitter_counts()[1] == [5]


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_every_refusal_changes_nothing(hip_libs):
    lib, T = hip_libs.load(3)
    invalid, unsupported = _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    uni = block(3, (8, 8, 8))
    sc = scene_of(uni)
    pipe, data = new_data(sc, particle_capacity=600)
    pipe.step(data, 2)
    data.sync()
    before = _digest(data)

    def refused(code, fn, *a, **kw):
        with pytest.raises(_ffi.WgsError) as err:
            fn(*a, **kw)
        assert err.value.code == code, str(err.value)
        return str(err.value)

    one = sub(uni, slice(0, 1))
    refused(invalid, data.add_particles, sub(uni, slice(0, 89)))                                  # beyond the capacity
    assert lib.wgs_add_particles(data._h, None, None, 1) == invalid and lib.wgs_add_particles(None, None, None, 0) == invalid
    refused(invalid, data.add_particles, one, models=np.array([3], np.uint8))                     # a model byte > 2
    heavier = one.copy()
    heavier.mass[:] *= np.float32(2.0)
    assert "uniform-material" in refused(unsupported, data.add_particles, heavier)                # other constants than the uniform ones
    plastic = sub(block(3, (2, 2, 2), plasticity=DruckerPrager.new(1e6, 0.25), phase=None), slice(0, 1))
    assert "plastic state" in refused(unsupported, data.add_particles, plastic)                   # plasticity on data without plastic state
    breaking = sub(block(3, (2, 2, 2), phase=ParticlePhase(1.0, 1.5)), slice(0, 1))
    assert "plastic state" in refused(unsupported, data.add_particles, breaking)                  # a phase that fractures, likewise
    ok = dict(lo=(6.0, 9.0, 6.0), count=(2, 2, 2), spacing=0.5)
    E = _ffi.emitter_type(T, 3)
    raw = (E * 9)()
    assert lib.wgs_set_emitters(data._h, raw, 9) == invalid and lib.wgs_set_emitters(data._h, None, 1) == invalid
    data.set_emitters([Emitter(one, **ok)])
    def current():
        got, n = (E * 8)(), C.c_uint32(0)
        assert lib.wgs_get_emitters(data._h, got, C.byref(n)) == 0 and n.value == 1
        arr = (E * 1)()
        C.memmove(arr, got, C.sizeof(E))
        return arr

    for field, value in (("period", 0), ("jitter", 0.75), ("jitter", float("nan")), ("model", 3), ("spacing", float("inf"))):
        arr = current()
        setattr(arr[0], field, value)
        assert lib.wgs_set_emitters(data._h, arr, 1) == invalid, field
    arr = current()
    arr[0].count[1] = 0
    assert lib.wgs_set_emitters(data._h, arr, 1) == invalid                                        # a count of 0
    arr[0].count[1] = 700
    assert lib.wgs_set_emitters(data._h, arr, 1) == invalid                                        # a batch beyond the capacity
    assert "uniform-material" in refused(unsupported, data.set_emitters, [Emitter(heavier, **ok)])
    assert "plastic state" in refused(unsupported, data.set_emitters, [Emitter(plastic, **ok)])
    assert len(data.emitters()) == 1 and data.emitters()[0].count == (2, 2, 2), "the refusals left the set alone"
    assert lib.wgs_get_emitters(data._h, None, None) == invalid and lib.wgs_get_emitter_counts(data._h, None, None) == invalid
    assert lib.wgs_get_particle_capacity(data._h, None) == invalid
    data.set_emitters(None)
    assert _digest(data) == before and data.n == 512
    # plastic data: a fluid label is refused; uniform plasticity parameters are held bit for bit
    sand = block(3, (8, 8, 8), plasticity=DruckerPrager.new(1e6, 0.25), phase=None)
    pipe, pdata = new_data(scene_of(sand), particle_capacity=600)
    one = sub(sand, slice(0, 1))
    assert "WGS_MODEL_FLUID" in refused(unsupported, pdata.add_particles, one, models=np.array([MODEL_FLUID], np.uint8))
    assert "WGS_MODEL_FLUID" in refused(unsupported, pdata.set_emitters, [Emitter(one, model=MODEL_FLUID, **ok)])
    other = one.copy()
    other.dp[:, 1] *= np.float32(1.25)
    assert "h0..h3" in refused(unsupported, pdata.add_particles, other)
    other = one.copy()
    other.dp[:, 5] *= np.float32(1.25)
    assert "uniform ones" in refused(unsupported, pdata.add_particles, other)
    pdata.add_particles(one)
    assert pdata.n == 513
    # sharded data
    slab_scene = scene_of(cloud(3, 600, two_materials=False, seed=90))
    shards, _ = lockstep_slabs(pipe, slab_scene, 2)
    cnt, n = (C.c_uint64 * 8)(), C.c_uint32(0)
    for s in shards:
        raw1 = (T.Particle * 1)()
        assert lib.wgs_add_particles(s._h, raw1, None, 1) == unsupported and b"single-domain data only" in lib.wgs_last_error()
        assert lib.wgs_set_emitters(s._h, None, 0) == unsupported and lib.wgs_get_emitters(s._h, (E * 8)(), C.byref(n)) == unsupported
        assert lib.wgs_get_emitter_counts(s._h, cnt, cnt) == unsupported


# ------------------------------------------------------------------------------------------------ 7. the scenes
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", ["faucet", "sand_pour"])
def test_the_pouring_scenes(hip_libs, name, dim):
    sc = getattr(scenes, name)(dim, batches=5)
    em = sc["emitters"][0]
    n0, h = sc["particles"].n, sc["cell_width"]
    pipe, data = new_data(sc)
    assert data.n == n0
    pipe.step(data, 40)
    data.sync()
    batches = ET.scheduled_batches(em, 40)
    assert batches == 5 and data.n == n0 + batches * em.batch_size == data.stats()["num_particles"] == data.particle_capacity
    assert data.emitter_counts() == ([5 * em.batch_size], [0])
    diag = data.diagnostics()
    assert diag.num_nonfinite == 0 and diag.num_particles == data.n
    pos = data.read_positions().astype(np.float64)
    for f, w in enumerate(sc.get("walls") or []):
        if w is None:
            continue
        k = f // 2
        if f % 2 == 0:
            assert pos[:, k].min() >= (w.plane - 1.5) * h, (f, pos[:, k].min())
        else:
            assert pos[:, k].max() <= (w.plane + 1.5) * h, (f, pos[:, k].max())
    if name == "sand_pour":
        assert pos[:, 1].min() >= (2.0 - 1.5) * h                           # the floor collider's top is at 2 h
    # what was poured has moved down from where it was emitted: the centre of mass of the emitted particles lies below the nozzle
    poured = pos[n0:]
    nozzle_bottom = em.lo[1]
    assert poured.shape[0] == 5 * em.batch_size and poured[:, 1].mean() < nozzle_bottom
    if name == "faucet":                                                     # ... and so has the fluid's mass moment over its mass
        mm, m = diag.sums["mass_moment"].value, diag.sums["mass"].value[0]
        assert mm[1] / m < nozzle_bottom and abs(mm[1] / m - poured[:, 1].mean()) < 1e-3 * abs(poured[:, 1].mean())
