"""-m gpu: the Lagrangian field output (MpmData.particle_fields / particle_fields_device; include/wgsparkl_hip.h) on the device —
every record against the fp64 truth of tests/field_truth.py at hard deformations, the same arithmetic as the step (bit for bit
without plastic state), the caller's order through the sort and both ping-pong sides, the last wave and workgroup, read-only, the
fluid and the per-particle table, refusals.

Every comparison goes through helpers.report_margin; figures measured on one MI355X are in profiles/r22_fields_margins.json."""
import contextlib
import ctypes as C
import dataclasses
import zlib

import numpy as np
import pytest

import devmath_truth as T
import field_truth as FT
from helpers import debug, new_data, pipeline, report_margin
from test_gpu_constitutive import CASES, _scene
from wgsparkl_amd import _ffi
from wgsparkl_amd.models import MODEL_COROTATED, MODEL_FLUID, MODEL_NEO_HOOKEAN
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import ParticleSet, SimulationParams

pytestmark = pytest.mark.gpu

H, DT = FT.H, FT.DT
ARRAYS = [f.name for f in dataclasses.fields(ParticleSet) if f.name != "dim"]
FIELDS = ("stress", "mean_stress", "von_mises", "volume_ratio", "stretch", "model")
UNSUPPORTED, INVALID = _ffi.ERR_UNSUPPORTED, _ffi.ERR_INVALID_ARGUMENT
CANARY = 0x5a5a5a5a


def _scene_of(ps, model, **kw):
    return dict(particles=ps, params=SimulationParams(gravity=(0.0,) * ps.dim, dt=DT), colliders=[], cell_width=H, grid_capacity=2048,
                model=int(model), **kw)


def _device_fields(data, extra=0):
    """particle_fields_device into a canary-filled device buffer of n + extra records -> its words [n + extra, words] uint32"""
    import torch
    words = C.sizeof(data.T.ParticleField) // 4
    buf = torch.full(((data.n + extra) * words,), CANARY, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    data.particle_fields_device(buf.data_ptr())
    data.sync()
    return buf.cpu().numpy().view(np.uint32).reshape(data.n + extra, words)


def _check(tag, data, inp):
    fields = data.particle_fields()
    fails = FT.check_fields(tag, inp, fields)
    assert not fails, "\n".join(fails[:12])
    return fields


# ------------------------------------------------------------------------------------------------ 1 catalogue, no substep
@pytest.mark.parametrize("per_particle", [False, True], ids=["uniform", "per_particle"])
@pytest.mark.parametrize("model", [MODEL_COROTATED, MODEL_NEO_HOOKEAN])
@pytest.mark.parametrize("dim", [3, 2])
def test_catalogue_before_the_first_substep(hip_libs, monkeypatch, dim, model, per_particle):
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    ps = FT.catalogue_particles(dim, model, per_particle)
    sc = _scene_of(ps, model)
    _, data = new_data(sc)
    fields = _check(f"catalogue model {model} {'per-particle' if per_particle else 'uniform'} {dim}d", data, FT.Inputs.of(ps, model))
    assert np.array_equal(fields.model, np.full(ps.n, model, np.uint32))
    if dim == 3 and not per_particle:
        # the uniform-material layout (F[8] in XM.w, the four constants kernel arguments) against the general one: the same records
        with debug(monkeypatch, "NO_UNIFORM"):
            general = new_data(sc)[1].particle_fields()
        assert general.raw.tobytes() == fields.raw.tobytes(), "the uniform-material layout changes a record"


# ------------------------------------------------------------------------------------------------ 2 the same arithmetic as the step
def _coeff(init_volume):
    """fl(fl(V0 * inv_d) * dt) with inv_d = 4 / h^2 = 4 at h = 1: the factor of tau in C' = grad m - tau (V0 inv_d dt)"""
    return ((init_volume.astype(np.float32) * np.float32(4.0)).astype(np.float32) * np.float32(DT)).astype(np.float32)


def _assert_at_rest(got, ps):
    assert np.array_equal(got.vel, np.zeros_like(got.vel)), "vel != 0: the zero-momentum construction did not hold"
    assert np.array_equal(got.pos, ps.pos), "pos moved"


def _elastic_case(name, dim):
    if name in ("elastic_corotated_uniform", "elastic_neo_hookean_per_particle"):
        sc, _ = _scene(dim, *CASES[name][:6], seed=zlib.crc32(name.encode()) % 1000 + dim)
        return sc
    if name == "fluid":
        return _scene_of(FT.fluid_particles(dim), MODEL_FLUID, fluid_gamma=7.0)
    ps, table = FT.mixed_particles(dim)
    return _scene_of(ps, MODEL_NEO_HOOKEAN, fluid_gamma=7.0, models=table)


@pytest.mark.parametrize("name", ["elastic_corotated_uniform", "elastic_neo_hookean_per_particle", "fluid", "mixed_table"])
@pytest.mark.parametrize("dim", [3, 2])
def test_the_stress_is_the_tau_of_the_step_bit_for_bit(hip_libs, monkeypatch, dim, name):
    """vel = 0, affine = 0, gravity = 0 (tests/test_gpu_constitutive.py): the velocity gradient of the substep is exactly 0, F stays,
    and affine_out = 0 m - tau coeff = -fl(tau coeff). The read-out of the state after the substep is that tau."""
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    sc = _elastic_case(name, dim)
    ps = sc["particles"]
    _, data = new_data(sc)
    before = data.particle_fields()
    data.pipeline.step(data, 1)
    data.sync()
    got = data.read_particles()
    _assert_at_rest(got, ps)
    models = sc.get("models", sc["model"])
    fields = _check(f"step arithmetic {name} {dim}d", data, FT.Inputs.of(got, models, sc.get("fluid_gamma", 7.0)))
    assert np.array_equal(got.def_grad, ps.def_grad), "F changed"
    for f in FIELDS:   # (by value: the substep may turn a -0 of F into +0)
        assert np.array_equal(getattr(before, f), getattr(fields, f)), f"F stays but {f} of the record does not"
    want = -(fields.stress * _coeff(got.init_volume)[:, None, None])
    assert want.dtype == np.float32
    affine = T.mat(got.affine, dim)
    assert np.abs(affine).max() > 0
    assert np.array_equal(affine, want), f"{int((affine != want).any((1, 2)).sum())} of {ps.n} particles: affine_out != -(stress * coeff)"


@pytest.mark.parametrize("name", ["plastic_mode2_corotated", "plastic_mode1_fracture_neo_hookean", "plastic_mode0_per_particle_state"])
@pytest.mark.parametrize("dim", [3, 2])
def test_the_stress_of_drucker_prager_data_is_the_tau_of_the_step_to_rounding(hip_libs, monkeypatch, dim, name):
    """The stored F is the projected elastic part; the step took tau from the SVD its projection maintained, the read-out from a fresh
    one: two fp32 evaluations, each inside C_TAU u tau_scales of the truth. |affine_out + stress coeff| <= coeff 2 C_TAU u tau_scales."""
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    model, plastic, mode = CASES[name][:3]
    assert plastic and CASES[name][-1] is None
    sc, _ = _scene(dim, *CASES[name][:6], seed=zlib.crc32(name.encode()) % 1000 + dim)
    ps = sc["particles"]
    rng = np.random.default_rng(11 + dim)
    state = np.tile(np.array([1.0, 1.0, 0.0], np.float32), (ps.n, 1))
    if mode == 0:
        state = np.stack([rng.uniform(0.8, 1.2, ps.n), rng.uniform(0.0, 2.0, ps.n), rng.uniform(-0.2, 0.2, ps.n)], 1).astype(np.float32)
    _, data = new_data(sc)
    data.set_plastic_state(state)
    data.pipeline.step(data, 1)
    data.sync()
    got = data.read_particles()
    _assert_at_rest(got, ps)
    assert (got.def_grad != ps.def_grad).any(), "nothing was projected"
    tag = f"step arithmetic {name} {dim}d"
    fields = _check(tag, data, FT.Inputs.of(got, model))
    coeff = _coeff(got.init_volume).astype(np.float64)
    F = T.mat(got.def_grad, dim).astype(np.float64)
    s64 = T.svd_lapack(got.def_grad)[1]
    scale = T.tau_scales(model, F, got.lambda_.astype(np.float64), got.mu.astype(np.float64), s64)
    err = np.linalg.norm(T.mat(got.affine, dim).astype(np.float64) + fields.stress.astype(np.float64) * coeff[:, None, None], axis=(1, 2))
    bound = coeff * 2 * T.C_TAU * T.U32 * scale
    uniq = T.tau_unique(s64) if model == MODEL_COROTATED else np.ones(ps.n, bool)
    w = int(np.argmax(np.where(uniq, err / bound, 0.0)))
    report_margin(f"{tag}: |affine_out + stress coeff| (scale coeff tau_scales)", float(err[w]), float(bound[w]), n=int(uniq.sum()))
    bad = uniq & ~(err <= bound)
    assert not bad.any(), f"{int(bad.sum())} particles over the bound (first #{int(np.argmax(bad))}: {err[np.argmax(bad)]:.3e} > {bound[np.argmax(bad)]:.3e})"


# ------------------------------------------------------------------------------------------------ 3 order and ping-pong
def _flight(dim, steps):
    _, data = new_data(FT.flying_cloud(dim))
    data.pipeline.step(data, steps)
    data.sync()
    return data


@pytest.mark.parametrize("dim", [3, 2])
def test_records_are_in_the_callers_order_on_both_sides(hip_libs, monkeypatch, dim):
    """30 substeps of a cloud flying through the grid: the sort moves particles every substep and the state alternates between the two
    buffers. Record i is particle i of read_particles() at 29 and at 30 substeps; the host form is the device form; the two-pass G2P
    leaves the same bits."""
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    data = _flight(dim, 29)
    raws = []
    for steps in (29, 30):
        got = data.read_particles()
        fields = _check(f"flying cloud {dim}d after {steps}", data, FT.Inputs.of(got, MODEL_COROTATED))
        assert fields.raw.tobytes() == _device_fields(data).tobytes(), "host form != device form"
        raws.append(fields.raw)
        ids = data.read_blocks()[3]
        assert not np.array_equal(ids, np.arange(data.n)), "the sort left the upload order: the test does not show the scatter"
        if steps == 29:
            data.pipeline.step(data, 1)
            data.sync()
    assert raws[0].tobytes() != raws[1].tobytes()
    with debug(monkeypatch, "G2P_TWO_PASSES"):
        two = _flight(dim, 29)
        two.pipeline.step(two, 1)
        two.sync()
        assert two.particle_fields().raw.tobytes() == raws[1].tobytes(), "G2P_TWO_PASSES changes a record"


# ------------------------------------------------------------------------------------------------ 4 tail sizes
@pytest.mark.parametrize("n", FT.TAILS)
@pytest.mark.parametrize("dim", [3, 2])
def test_the_last_wave_and_the_last_workgroup(hip_libs, monkeypatch, dim, n):
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    model = n % 2
    ps = FT.catalogue_particles(dim, model, True, n=n, seed=n)
    _, data = new_data(_scene_of(ps, model))
    fields = _check(f"tail n={n} {dim}d", data, FT.Inputs.of(ps, model))
    words = _device_fields(data, extra=8)
    assert words[:n].tobytes() == fields.raw.tobytes()
    assert (words[n:] == CANARY).all(), "a word beyond n records was written"
    assert (fields.raw != CANARY).any(1).all(), "a record was left unwritten"


# ------------------------------------------------------------------------------------------------ 5 read-only
def _same_particles(a, b, what):
    for f in ARRAYS:
        x, y = np.ascontiguousarray(getattr(a, f)), np.ascontiguousarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, f)


@pytest.mark.parametrize("kind", ["cloud3", "cloud2", "block_in_fluid3"])
def test_asking_changes_nothing(hip_libs, monkeypatch, kind):
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    dim = int(kind[-1])
    make = (lambda: FT.flying_cloud(dim)) if kind.startswith("cloud") else (lambda: FT.small_block_in_fluid(dim))

    def digest(data):
        return data.diagnostics(_ffi.DIAG_DIGEST).digest

    def run(ask):
        _, data = new_data(make())
        for k in range(20):
            data.pipeline.step(data, 1)
            if ask:
                (data.particle_fields if k % 2 else lambda: _device_fields(data))()
        data.sync()
        return data

    asked, plain = run(True), run(False)
    assert digest(asked) == digest(plain)
    _same_particles(asked.read_particles(), plain.read_particles(), "20 substeps with a call after each")
    # one call: digest, every field of read_particles and the device memory of the data stay
    d0, p0, bytes0 = digest(asked), asked.read_particles(), asked.stats()["device_bytes"]
    asked.particle_fields()
    _device_fields(asked)
    assert digest(asked) == d0 and asked.stats()["device_bytes"] == bytes0 == plain.stats()["device_bytes"]
    _same_particles(asked.read_particles(), p0, "across a call")


# ------------------------------------------------------------------------------------------------ 6 fluid
def test_tait_fluid_block_after_24_substeps(hip_libs, monkeypatch):
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    sc = FT.small_tait_block()
    _, data = new_data(sc)
    data.pipeline.step(data, 24)
    data.sync()
    got = data.read_particles()
    J = got.def_grad[:, 0]
    assert (J != 1.0).any() and (J > 0).all(), "the block should have been compressed by its weight"
    fields = _check("tait_fluid_block after 24", data, FT.Inputs.of(got, MODEL_FLUID, sc["fluid_gamma"]))
    assert np.array_equal(fields.model, np.full(data.n, MODEL_FLUID, np.uint32))
    assert np.array_equal(fields.volume_ratio, J)
    off = fields.stress[:, ~np.eye(3, dtype=bool)]
    assert np.array_equal(off, np.zeros_like(off)), "the pressure part alone: no shear stress"


@pytest.mark.parametrize("dim", [3, 2])
def test_block_in_fluid_every_particle_under_its_own_model(hip_libs, monkeypatch, dim):
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    sc = FT.small_block_in_fluid(dim)
    _, data = new_data(sc)
    data.pipeline.step(data, 24)
    data.sync()
    got = data.read_particles()
    table = data.read_particle_models()
    assert np.array_equal(table, sc["models"])
    fields = _check(f"block_in_fluid {dim}d after 24", data, FT.Inputs.of(got, table, sc["fluid_gamma"]))
    assert np.array_equal(fields.model, sc["models"].astype(np.uint32))
    fl = table == MODEL_FLUID
    assert fl.any() and (~fl).any()
    assert (fields.stretch[fl] == fields.stretch[fl][:, :1]).all(), "a fluid particle is drawn isotropically"
    assert (np.abs(fields.stress[~fl]).max((1, 2)) > 0).any() and (got.def_grad[fl][:, 0] != 1.0).any()


# ------------------------------------------------------------------------------------------------ 7 refusals
@pytest.mark.parametrize("dim", [3, 2])
def test_sharded_data_and_null_outputs_are_refused(hip_libs, monkeypatch, dim):
    import torch
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    sc = FT.flying_cloud(dim)
    pipe = pipeline(dim)
    lib, T_ = pipe.lib, pipe.T
    words = C.sizeof(T_.ParticleField) // 4
    out = np.full((sc["particles"].n, words), CANARY, np.uint32)
    dev = torch.full((sc["particles"].n * words,), CANARY, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    pout = out.ctypes.data_as(C.POINTER(T_.ParticleField))
    shards, _ = lockstep_slabs(pipe, sc, 2)
    for s in shards:
        for call in (lambda: lib.wgs_read_particle_fields(s._h, pout), lambda: lib.wgs_read_particle_fields_device(s._h, C.c_void_p(dev.data_ptr()))):
            assert call() == UNSUPPORTED
            assert b"sharded" in lib.wgs_last_error()
    _, data = new_data(sc)
    for call in (lambda: lib.wgs_read_particle_fields(data._h, None), lambda: lib.wgs_read_particle_fields_device(data._h, None),
                 lambda: lib.wgs_read_particle_fields_device(data._h, C.c_void_p(dev.data_ptr() + 4))):     # (not aligned to a vector)
        assert call() == INVALID
        assert lib.wgs_last_error()
    data.sync()
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (dev.cpu().numpy().view(np.uint32) == CANARY).all(), "a refused call wrote something"
    for s in shards:
        s.close()
