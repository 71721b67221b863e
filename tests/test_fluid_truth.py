"""-m "not gpu": the fluid model's truth (tests/fluid_truth.py) checked against what the model claims of itself, and the public
surface of MODEL_FLUID: header, ctypes binding and both built libraries."""
import os
import re

import numpy as np
import pytest

import fluid_truth as ft
from wgsparkl_amd import scenes
from wgsparkl_amd.models import MODEL_FLUID, FluidCoefficients
from wgsparkl_amd.solver import ParticleSet, SimulationParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "wgsparkl_hip.h")).read()


def _block(dim, n_side=10, bulk=1.0e5, visc=0.0, jitter=0.05, seed=3):
    h = 1.0
    pos = scenes.lattice((n_side,) * dim, (6.0,) * dim, h, jitter, seed=seed)
    return ParticleSet.uniform(pos, h / 4.0, 1000.0, FluidCoefficients(bulk, visc))


# ------------------------------------------------------------------------------------------------ the formulae
@pytest.mark.parametrize("gamma", [7.0, 3.5])
def test_pressure_stress_is_the_derivative_of_psi(gamma):
    """mu = 0: tau = J dPsi/dJ I, by central differences of Psi in fp64."""
    J = np.linspace(0.6, 1.6, 41)
    lam = np.full_like(J, 3.0e5)
    G = np.zeros((len(J), 3, 3))
    tau = ft.kirchhoff(J, G, lam, np.zeros_like(J), gamma)
    e = 1.0e-6
    dpsi = (ft.psi(J + e, lam, gamma) - ft.psi(J - e, lam, gamma)) / (2 * e)
    for k in range(3):
        assert np.allclose(tau[:, k, k], J * dpsi, rtol=1e-7, atol=1e-9 * 3.0e5)
    assert np.all(tau[:, 0, 1] == 0) and np.all(tau[:, 2, 1] == 0)
    assert abs(ft.psi(np.array([1.0]), np.array([3.0e5]), gamma)[0]) == 0.0
    # -dPsi/dJ = p, and dp/dJ = -lambda at J = 1
    assert np.allclose(-dpsi, ft.pressure(J, lam, gamma), rtol=1e-7, atol=1e-9 * 3.0e5)
    dp = (ft.pressure(np.array([1.0 + e]), lam[:1], gamma) - ft.pressure(np.array([1.0 - e]), lam[:1], gamma)) / (2 * e)
    assert abs(dp[0] / -3.0e5 - 1.0) < 1e-8


@pytest.mark.parametrize("dim", [2, 3])
def test_j_update_is_the_determinant_of_the_f_form_update(dim):
    """J' = det of F <- F + (G dt) F, for F = diag(J, 1[, 1]) and for the isotropic F = J^(1/d) I alike."""
    rng = np.random.default_rng(5)
    n, dt = 200, 1.0 / 1200.0
    J = rng.uniform(0.7, 1.4, n)
    G = rng.normal(0.0, 30.0, (n, dim, dim))
    Jn = ft.advance_j(J, G, dt)
    eye = np.eye(dim)
    Fd = np.tile(eye, (n, 1, 1))
    Fd[:, 0, 0] = J
    Fi = (J ** (1.0 / dim))[:, None, None] * eye
    for F in (Fd, Fi):
        Fn = F + (G * dt) @ F
        assert np.allclose(np.linalg.det(Fn), Jn, rtol=1e-13, atol=0)
    assert np.array_equal(np.linalg.det(ft._mat(ft.fluid_def_grad(J, dim), dim)), J)   # diag(J, 1, 1): its determinant is J itself


def test_pressure_term_is_lambda_ln_j_to_first_order():
    """-Jc p - lambda ln J = O((J - 1)^2): halving J - 1 quarters the difference."""
    lam, gamma = np.array([1.0e7]), 7.0
    diff = []
    for e in (4e-3, 2e-3, 1e-3, -1e-3, -2e-3):
        J = np.array([1.0 + e])
        diff.append(float((-J * ft.pressure(J, lam, gamma) - lam * np.log(J))[0]))
    assert abs(diff[0] / diff[1] - 4.0) < 0.1 and abs(diff[1] / diff[2] - 4.0) < 0.1 and abs(diff[4] / diff[3] - 4.0) < 0.1
    assert abs(diff[2]) < 1.0e7 * 1e-3 ** 2 * 10.0     # the coefficient of (J - 1)^2 is a few lambda


# ------------------------------------------------------------------------------------------------ the substep
@pytest.mark.parametrize("dim", [2, 3])
def test_uniform_motion_of_a_compressed_block_keeps_linear_momentum(dim):
    ps = _block(dim, visc=40.0)
    ps.vel[:] = np.array([0.7, -0.4, 0.3], np.float32)[:dim]
    ps.def_grad[:, 0] = 0.97                                             # uniformly compressed: it expands from the first substep
    st = ft.FluidState(ps, SimulationParams(gravity=(0.0,) * dim, dt=1.0 / 1200.0), 1.0, gamma=7.0)
    assert np.allclose(st.J, 0.97, rtol=1e-7)
    p0 = st.momentum()
    for _ in range(12):
        st.step(1)
        assert np.max(np.abs(st.momentum() - p0)) <= 1e-12 * np.max(np.abs(p0))
    assert st.J.max() > 0.9701, "the block should have expanded"


def _shear_run(visc, steps=20):
    ps = _block(3, n_side=12, bulk=1.0e5, visc=visc)
    c = ps.pos.mean(0)
    ps.vel[:, 0] = (ps.pos[:, 1] - c[1]) * 2.0                          # shear du/dy = 2 / s
    params = SimulationParams(gravity=(0.0, 0.0, 0.0), dt=1.0 / 1200.0)
    st = ft.FluidState(ps, params, 1.0, gamma=7.0)
    psi0 = float(np.sum(st.vol * ft.psi(st.J, st.lam, st.gamma)))
    work, kin = 0.0, []
    h2q = 1.0 / 4.0
    for _ in range(steps):
        st.step(1)
        tau = ft.kirchhoff(st.J, st.last_grad, st.lam, st.mu, st.gamma)
        work += float(np.sum(st.vol * np.einsum("nrc,nrc->n", tau, st.last_grad))) * st.dt   # what the stress takes out of the motion
        aff = 0.5 * h2q * np.sum(np.sum(st.C ** 2, 1) / st.mass)
        kin.append(st.kinetic() + float(aff))
    stored = float(np.sum(st.vol * ft.psi(st.J, st.lam, st.gamma))) - psi0
    return np.array(kin), work, stored


def test_viscosity_dissipates_and_pressure_does_not():
    """Shear flow: with mu > 0 the kinetic energy (particle + affine, what P2G puts on the grid) falls in every substep; with mu = 0
    whatever the stress takes out of the motion is stored in Psi (dPsi/dJ = -p), none of it is lost."""
    kin_v, work_v, stored_v = _shear_run(200.0)
    kin_0, work_0, stored_0 = _shear_run(0.0)
    assert np.all(np.diff(kin_v) < 0.0)
    dissipated = work_v - stored_v
    assert dissipated > 0.0 and dissipated > 0.05 * (kin_v[0] - kin_v[-1])
    # mu = 0: the stress work equals the change of the stored energy up to the O(dt) error of the explicit update
    # (kinetic energy still falls at the free faces, where the shear compresses the block: it is in Psi, not gone)
    assert abs(work_0 - stored_0) <= 1e-3 * dissipated


@pytest.mark.parametrize("dim", [2, 3])
def test_fp32_restatement_tracks_the_truth(dim):
    ps = _block(dim, visc=20.0)
    c = ps.pos.mean(0)
    ps.vel[:] = ((c - ps.pos) * 1.5).astype(np.float32)
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1.0 / 1200.0)
    a, b = ft.FluidState(ps, params, 1.0, 7.0, np.float64), ft.FluidState(ps, params, 1.0, 7.0, np.float32)
    a.step(10)
    b.step(10)
    assert b.pos.dtype == np.float32 and b.J.dtype == np.float32 and b.C.dtype == np.float32
    assert np.max(np.abs(a.J - b.J)) < 1e-5 and np.max(np.abs(a.pos - b.pos)) < 1e-4
    assert a.J.min() < 0.99
    cells, vm = a.grid_records()
    assert len(cells) % 64 == 0 and np.all(np.isfinite(vm))


# ------------------------------------------------------------------------------------------------ the public surface
def test_header_and_binding_carry_the_fluid(hip_libs):
    assert re.search(r"WGS_MODEL_FLUID = 2\b", HEADER)
    assert re.search(r"^wgs_status wgs_set_fluid_eos\(wgs_data \*data, float gamma\);", HEADER, re.M)
    assert "wgs_set_fluid_eos" in hip_libs.EXPORTS and MODEL_FLUID == 2
    for dim in (2, 3):
        lib, _ = hip_libs.load(dim)
        assert hasattr(lib, "wgs_set_fluid_eos"), f"libwgsparkl{dim}d_hip.so does not export wgs_set_fluid_eos"
        # argument checks that need no device: NULL data
        assert lib.wgs_set_fluid_eos(None, 7.0) == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_set_constitutive_model(None, MODEL_FLUID) == hip_libs.ERR_INVALID_ARGUMENT


def test_scenes_for_the_fluid():
    a = scenes.fluid_block(16, 16, 16)
    b = scenes.tait_fluid_block(16, 16, 16, viscosity=3.0, gamma=5.0)
    assert np.array_equal(a["particles"].pos, b["particles"].pos) and np.array_equal(a["global_ids"], b["global_ids"])
    assert a["model"] == 1 and b["model"] == MODEL_FLUID and b["fluid_gamma"] == 5.0
    assert np.all(b["particles"].mu == np.float32(3.0)) and np.array_equal(a["particles"].lambda_, b["particles"].lambda_)
    d = scenes.dam_break()
    assert d["model"] == MODEL_FLUID and len(d["colliders"]) == 2 and d["particles"].n == 24 * 40 * 16
    assert d["particles"].pos[:, 0].min() > 8.0 and d["particles"].pos[:, 1].min() > 2.0   # outside the wall and above the floor
