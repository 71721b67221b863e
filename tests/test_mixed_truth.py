"""-m "not gpu": the truth of per-particle constitutive models (tests/mixed_truth.py) against the truths it is assembled from, the
fairness of the coupled scenes the GPU parity test runs, and the public surface (header, bindings, scene)."""
import os
import re

import numpy as np
import pytest

import fluid_truth as ft
import mixed_truth as mt
from gpu_common import GRID_V_TOL, PART_TOL
from helpers import rel_rms
from oracle.np_oracle import NpState
from wgsparkl_amd import scenes
from wgsparkl_amd.models import MODEL_FLUID, MODEL_PER_PARTICLE, ElasticCoefficients, FluidCoefficients, ParticlePhase
from wgsparkl_amd.solver import ParticleSet, SimulationParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()
U32 = 2.0 ** -24
# all-solid table, fp32, against the fp64 NpState: every field of a substep is a sum of ~200 rounded terms (3^D nodes x the ~8
# particles of a cell), a random walk of sqrt(200) ~ 14 roundings; four substeps ~ 60; 256 leaves a factor of four
SOLID32_ROUNDINGS = 256


def _block(dim, material, n_side=10, seed=3):
    h = 1.0
    pos = scenes.lattice((n_side,) * dim, (6.0,) * dim, h, 0.05, seed=seed)
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, material, phase=ParticlePhase(1.0, scenes.FLT_MAX))
    c = pos.mean(0)
    ps.vel[:] = ((c - pos) * 2.0).astype(np.float32)
    ps.vel[:, 0] += ((pos[:, 1] - c[1]) * 2.5).astype(np.float32)
    return ps


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("dim", [2, 3])
def test_all_fluid_table_is_the_fluid_truth(dim, dtype):
    ps = _block(dim, FluidCoefficients(1.0e5, 20.0))
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0)
    a = ft.FluidState(ps, params, 1.0, 5.0, dtype)
    b = mt.MixedState(ps, params, 1.0, np.ones(ps.n, bool), 0, 5.0, dtype)
    a.step(8)
    b.step(8)
    for f in ("pos", "vel", "J", "F", "C", "last_grad"):
        assert getattr(b, f).dtype == np.dtype(dtype)
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(a.grid["vel"], b.grid["vel"]) and np.array_equal(a.grid["mass"], b.grid["mass"])
    assert np.all(b.models() == MODEL_FLUID)


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("dim", [2, 3])
def test_all_solid_table_is_the_solid_truth(dim, model):
    """fp64: the same arithmetic as NpState, statement for statement — exact. fp32: within SOLID32_ROUNDINGS unit roundoffs of it
    (relative RMS) after four substeps."""
    ps = _block(dim, ElasticCoefficients.from_young_modulus(2.0e5, 0.3))
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0)
    ref = NpState(ps, params, 1.0, model)
    a = mt.MixedState(ps, params, 1.0, np.zeros(ps.n, bool), model, 7.0, np.float64)
    b = mt.MixedState(ps, params, 1.0, np.zeros(ps.n, bool), model, 7.0, np.float32)
    ref.step(4)
    a.step(4)
    b.step(4)
    for f in ("pos", "vel", "F", "C"):
        assert np.array_equal(getattr(a, f), getattr(ref, f)), f
    assert np.array_equal(a.grid["vel"], ref.grid["vel"])
    assert np.all(a.models() == model)
    assert np.abs(ref.F - np.eye(dim).reshape(-1)).max() > 1e-3, "the block should deform"
    for f in ("pos", "vel", "F"):
        err = rel_rms(getattr(b, f), getattr(ref, f))
        assert err <= SOLID32_ROUNDINGS * U32, (f, err / U32)


@pytest.mark.parametrize("solid_model", [0, 1])
@pytest.mark.parametrize("dim", [2, 3])
def test_coupled_scene_conserves_momentum_without_gravity(dim, solid_model):
    sc = mt.coupled_scene(dim, solid_model, "random", gravity=False)
    st = mt.MixedState(sc["particles"], sc["params"], 1.0, sc["fluid"], solid_model, sc["fluid_gamma"], np.float64)
    p0 = st.momentum()
    scale = float(np.sum(st.mass * np.linalg.norm(st.vel, axis=1)))        # (the shear and the converging field nearly cancel in the sum)
    for _ in range(mt.SUBSTEPS):
        st.step(1)
        assert np.max(np.abs(st.momentum() - p0)) <= 1e-12 * scale


@pytest.mark.parametrize("pattern", mt.PATTERNS)
@pytest.mark.parametrize("solid_model", [0, 1])
@pytest.mark.parametrize("dim", [2, 3])
def test_coupled_scenes_are_fair(dim, solid_model, pattern):
    """What the GPU parity test may assume of its scenes: the fp32 restatement itself stays within HALF of the tolerances the device is
    held to (`affine` has the project's escape and is exempt), the fluid compresses, the solid deforms enough for its stress to matter,
    and both kinds are there."""
    sc, s64, s32 = mt.coupled_truths(dim, solid_model, pattern)
    fl = sc["fluid"]
    assert 0.3 < fl.mean() < 0.7
    assert s64.J[fl].min() < 0.95, "the scene should compress"
    eye = np.eye(dim).reshape(-1)
    assert np.abs(s64.F[~fl] - eye).max() > 0.02, "the solid should deform"
    assert np.array_equal(s64.F[fl][:, 1:], np.tile(eye[1:], (int(fl.sum()), 1)))
    cells, vm = s64.grid_records()
    v32, m32 = s32.grid_at(cells.astype(np.int64))
    assert rel_rms(v32, vm[:, :dim]) <= 0.5 * GRID_V_TOL
    assert rel_rms(m32, vm[:, dim]) <= 0.5 * GRID_V_TOL
    assert rel_rms(s32.pos, s64.pos) <= 0.5 * PART_TOL
    assert rel_rms(s32.vel, s64.vel) <= 0.5 * PART_TOL
    assert rel_rms(s32.J[fl], s64.J[fl]) <= 0.5 * PART_TOL
    assert rel_rms(s32.F[~fl], s64.F[~fl]) <= 0.5 * PART_TOL
    if pattern == "plane":      # the interface cuts cells and blocks: both kinds share cells
        c = s64.cells0
        key = lambda a: [tuple(r) for r in a.tolist()]
        assert set(key(c[fl])) & set(key(c[~fl]))


# ------------------------------------------------------------------------------------------------ the public surface
def test_header_and_bindings_carry_the_per_particle_models(hip_libs):
    assert re.search(r"#define WGS_MODEL_PER_PARTICLE 3\b", HEADER) and MODEL_PER_PARTICLE == 3
    assert re.search(r"^wgs_status wgs_set_particle_models\(wgs_data \*data, const uint8_t \*models", HEADER, re.M)
    assert re.search(r"^wgs_status wgs_read_particle_models\(wgs_data \*data, uint8_t \*out\);", HEADER, re.M)
    invalid = hip_libs.ERR_INVALID_ARGUMENT
    for dim in (2, 3):
        lib, _ = hip_libs.load(dim)
        assert hasattr(lib, "wgs_set_particle_models") and hasattr(lib, "wgs_read_particle_models")
        # argument checks that need no device: NULL data
        assert lib.wgs_set_particle_models(None, None) == invalid and lib.wgs_read_particle_models(None, None) == invalid
        assert lib.wgs_set_constitutive_model(None, 0) == invalid


def test_block_in_fluid_scene():
    sc = scenes.block_in_fluid()
    ps, models = sc["particles"], sc["models"]
    assert models.dtype == np.uint8 and models.shape == (ps.n,)
    solid = models != MODEL_FLUID
    assert sc["solid_model"] in (0, 1) and np.all(models[solid] == sc["solid_model"]) and 0 < solid.sum() < ps.n
    assert sc["model"] == sc["solid_model"] and len(sc["colliders"]) >= 3
    # the block hangs above the fluid's surface, inside the tank; nothing starts inside a collider
    assert ps.pos[solid][:, 1].min() > ps.pos[~solid][:, 1].max()
    assert ps.pos[:, 1].min() > 2.0 and ps.pos[:, 0].min() > 8.0
    # the two materials carry their own coefficients
    assert np.all(ps.mu[~solid] == ps.mu[~solid][0]) and ps.lambda_[solid][0] != ps.lambda_[~solid][0]
    assert sorted(set(models.tolist())) == sorted({MODEL_FLUID, sc["solid_model"]})
    assert scenes.block_in_fluid(solid_model=0)["solid_model"] == 0
