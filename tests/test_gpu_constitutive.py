"""-m gpu: one substep of the product's G2P kernels read as a per-particle constitutive probe, checked particle by particle
against fp64 truth (tests/devmath_truth.py) at hard deformations.

Construction: vel = 0, affine = 0, gravity = 0. The grid then carries zero momentum, every grid velocity and the velocity
gradient are exactly 0, and after one substep
    F_out = F_in (or its Drucker-Prager projection),    affine_out = -tau(F_out) * V0 * (4 / h^2) * dt,
so the fracture decision, the projection and the stress of every particle are read off def_grad, dp_state, phase and
affine. That vel stays 0 and pos stays put is asserted first: it proves the construction held.

Discrete decisions (fracture s > max_stretch; Drucker-Prager trace ≷ 0, gamma ≤ 0 and the exact-equality all_zero) must
match the fp64 decision, except for particles whose fp64 decision quantities lie within a stated fp32 band of the
threshold; those are counted and the count bounded, and their result must be one of the legitimate outcomes. Pure
compression F = c I is such a case by construction: in fp32 log c summed d times and divided by d is not always log c, so
the kernel may keep F (gamma ≤ 0 on the cone branch) or project to the tip — both are computed in fp64 and accepted; the
fp32 oracle is no arbiter there (its SVD runs in fp64 and returns s = c exactly, the kernel gets sqrt(c^2) in fp32)."""
import contextlib
import zlib

import numpy as np
import pytest

import devmath_truth as T
from helpers import debug, new_data, report_margin
from wgsparkl_amd.models import MODEL_COROTATED, MODEL_NEO_HOOKEAN, DruckerPrager, ElasticCoefficients, ParticlePhase
from wgsparkl_amd.solver import Collider, ParticleSet, SimulationParams

pytestmark = pytest.mark.gpu

H = 1.0
DT = 1.0e-3
FRACTURE_STRETCH = 1.3
AMBIGUOUS_MAX = 0.02          # decision-ambiguous particles outside isotropic strain (pure compression / dilation), fraction


def _matrices(dim, plastic, n, rng):
    """n fp32 matrices drawn from the catalogue (plastic: the Drucker-Prager one, det F > 0), with their family names"""
    cat = T.dp_catalogue(dim, rng) if plastic else T.catalogue(dim, seed=4)
    names = np.concatenate([[k] * len(v) for k, v in cat.items()])
    F = np.concatenate(list(cat.values()))
    idx = np.concatenate([np.arange(len(F)), rng.integers(0, len(F), max(0, n - len(F)))])[:n]
    return F[idx], names[idx]


def _scene(dim, model, plastic, mode, per_particle, collider, fracture, seed):
    """`mode`: the uniform plasticity mode the library will pick (0: h0..h3 differ between particles, 1: only lambda / mu /
    max_stretch differ, 2: all equal). `fracture`: phase (1, max_stretch) — the particles stretched beyond it break and
    are projected; without it plastic particles carry phase None (0, -1)."""
    rng = np.random.default_rng(seed)
    n = 3000 if dim == 3 else 2000
    lo, hi = 2.0, 10.0
    pos = rng.uniform(lo, hi, (4 * n, dim))
    ball_c = np.array([6.0, 6.0, 12.5][:dim]) if dim == 3 else np.array([6.0, 12.5])
    ball_r = 2.5
    if collider:   # part of the cloud within a cell or two of the ball, none inside its reach (no penetration impulse)
        pos = pos[np.linalg.norm(pos - ball_c, axis=1) > ball_r + 0.5 * H]
    pos = pos[:n].astype(np.float32)
    dp = DruckerPrager.new(1e6, 0.25) if plastic else None
    phase = ParticlePhase(1.0, FRACTURE_STRETCH) if fracture else (None if plastic else ParticlePhase(1.0, -1.0))
    ps = ParticleSet.uniform(pos, H / 4.0, 10.0, ElasticCoefficients.from_young_modulus(1e5, 0.3), plasticity=dp, phase=phase)
    F, fam = _matrices(dim, plastic, n, rng)
    ps.def_grad[:] = F
    if per_particle:
        ps.lambda_[:] = (ps.lambda_ * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        ps.mu[:] = (ps.mu * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        ps.mass[:] = (ps.mass * rng.uniform(0.5, 1.5, n)).astype(np.float32)
        if model == MODEL_NEO_HOOKEAN:
            ps.mu[::5] = 0.0                                            # the C5 "fluid": pressure only
    elif model == MODEL_NEO_HOOKEAN and not plastic:
        ps.mu[:] = 0.0
    if plastic and mode == 0:
        ps.dp[:, 0] = (ps.dp[:, 0] * rng.uniform(0.9, 1.1, n)).astype(np.float32)
    if plastic and mode == 1:
        alt = DruckerPrager.new(3e5, 0.3).as_array()
        ps.dp[::3, 4:6] = alt[4:6]
        if fracture:
            ps.phase[1::4, 1] = np.float32(1.2)
    cols = [Collider.ball(ball_r, tuple(float(x) for x in ball_c))] if collider else []
    sc = dict(particles=ps, params=SimulationParams(gravity=(0.0,) * dim, dt=DT), colliders=cols, cell_width=H,
              grid_capacity=2048, model=model)
    return sc, fam


def _run(sc, state=None):
    pipe, data = new_data(sc)
    if state is not None:
        data.set_plastic_state(state)
    pipe.step(data, 1)
    data.sync()
    return data, data.read_particles()


CASES = {
    # name: (model, plastic, uni_dp mode, per-particle material, collider, fracture, WGS_DEBUG switch)
    "elastic_corotated_uniform": (MODEL_COROTATED, False, None, False, False, False, None),
    "elastic_neo_hookean_fluid_uniform": (MODEL_NEO_HOOKEAN, False, None, False, False, False, None),
    "elastic_neo_hookean_per_particle": (MODEL_NEO_HOOKEAN, False, None, True, False, False, None),
    "elastic_corotated_per_particle_collider": (MODEL_COROTATED, False, None, True, True, False, None),
    "plastic_mode2_corotated": (MODEL_COROTATED, True, 2, False, False, False, None),
    "plastic_mode2_fracture_collider": (MODEL_COROTATED, True, 2, False, True, True, None),
    "plastic_mode1_fracture_neo_hookean": (MODEL_NEO_HOOKEAN, True, 1, True, False, True, None),
    "plastic_mode0_per_particle_state": (MODEL_COROTATED, True, 0, True, False, False, None),
    "plastic_forced_mode0_collider": (MODEL_COROTATED, True, 2, False, True, True, "NO_UNIFORM"),
    "plastic_mode2_two_pass": (MODEL_COROTATED, True, 2, False, False, True, "G2P_TWO_PASSES"),
    "elastic_two_pass_collider": (MODEL_NEO_HOOKEAN, False, None, True, True, False, "G2P_TWO_PASSES"),
}


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_one_substep_constitutive_update_per_particle(hip_libs, monkeypatch, case, dim):
    dbg = CASES[case][-1]
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    with debug(monkeypatch, dbg) if dbg is not None else contextlib.nullcontext():
        _check_case(case, dim)


def _check_case(case, dim):
    model, plastic, mode, per_particle, collider, fracture, _ = CASES[case]
    sc, fam = _scene(dim, model, plastic, mode, per_particle, collider, fracture, seed=zlib.crc32(case.encode()) % 1000 + dim)
    ps = sc["particles"]
    n = ps.n
    rng = np.random.default_rng(11 + dim)
    state_in = np.tile(np.array([1.0, 1.0, 0.0], np.float32), (n, 1))
    if case == "plastic_mode0_per_particle_state":
        state_in = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.0, 2.0, n), rng.uniform(-0.2, 0.2, n)], 1).astype(np.float32)
    data, got = _run(sc, state_in if plastic else None)
    tag = f"{case} {dim}d"

    # the construction: nothing moves
    assert np.array_equal(got.vel, np.zeros_like(got.vel)), "vel != 0: the zero-momentum construction did not hold"
    assert np.array_equal(got.pos, ps.pos), "pos moved"
    if collider:
        assert (got.cdf_affinity != 0).sum() > 0.02 * n, "the collider is not felt by the cloud"
        assert data.stats()["num_near_collider_blocks"] > 0

    F_in = T.mat(ps.def_grad, dim)
    F_out = T.mat(got.def_grad, dim)
    svd_in = T.svd_lapack(ps.def_grad)
    s_in = svd_in[1]
    a_in, smax_in, _ = T.sv_stats(s_in)

    # fracture: the fp64 decision, except within the band of the threshold
    phase_in = ps.phase[:, 0].astype(np.float64)
    max_stretch = ps.phase[:, 1].astype(np.float64)
    breakable = (phase_in > 0) & (max_stretch > 0)
    smax_signed = s_in.max(1)
    broken64 = breakable & (smax_signed > max_stretch)
    amb_frac = breakable & (np.abs(smax_signed - max_stretch) <= T.C_DEC * T.U32 * smax_in)
    phase_gpu = got.phase[:, 0]
    want_phase = np.where(broken64, 0.0, phase_in)
    wrong_phase = (phase_gpu != want_phase) & ~amb_frac
    assert np.array_equal(got.phase[:, 1], ps.phase[:, 1]), "max_stretch changed"
    assert not wrong_phase.any(), f"{tag}: phase differs from the fp64 fracture decision for {int(wrong_phase.sum())} particles " \
                                  f"(first #{int(np.argmax(wrong_phase))}: s = {s_in[np.argmax(wrong_phase)]}, max_stretch " \
                                  f"{max_stretch[np.argmax(wrong_phase)]}, phase {phase_gpu[np.argmax(wrong_phase)]})"
    if fracture:
        assert 0 < int(broken64.sum()) < int(breakable.sum()), "fracture: some particles must break and some must not"

    # Drucker-Prager: particles with phase 0 after the fracture test and lambda != 0
    dpp = (phase_gpu == 0.0) & (ps.dp[:, 4] != 0.0)
    plastic_amb = np.zeros(n, bool)
    if dpp.any():
        idx = np.nonzero(dpp)[0]
        res = T.dp_outcomes64(ps.dp[idx].astype(np.float64), state_in[idx].astype(np.float64), F_in[idx],
                              tuple(x[idx] for x in svd_in))
        allowed = T.dp_allowed(res)
        plastic_amb[idx] = [len(a) > 1 for a in allowed]
        worst, fails = 0.0, []
        for k, i in enumerate(idx):
            changed = not (np.array_equal(got.def_grad[i], ps.def_grad[i]) and np.array_equal(got.dp_state[i], state_in[i]))
            br, w = T.dp_match(res, k, changed, F_out[i], got.dp_state[i].astype(np.float64), np.linalg.norm(F_in[i]))
            if br is None or not w <= 1.0:
                fails.append(f"#{i} ({fam[i]}): changed={changed} matches none of {sorted(allowed[k])} (best {br}: {w:.3g} x bound; "
                             f"fp64 branch {res['branch'][k]}, trace {res['tr'][k]:.3e}, gamma {res['gamma'][k]:.3e})")
            else:
                worst = max(worst, w)
        report_margin(f"{tag}: Drucker-Prager F / state, worst error / bound (branch-matched)", worst, 1.0, n=int(dpp.sum()))
        assert not fails, f"{tag}: {len(fails)} of {int(dpp.sum())} projected particles off:\n" + "\n".join(fails[:12])
    # everything not projected keeps F and its state bit for bit
    keep = ~dpp
    assert np.array_equal(got.def_grad[keep], ps.def_grad[keep]), f"{tag}: F changed without a projection"
    if plastic:
        assert np.array_equal(got.dp_state[keep], state_in[keep]), f"{tag}: plastic state changed without a projection"

    # the decisions the test could not hold to fp64: counted and bounded (pure compression is ambiguous by construction)
    amb = amb_frac | plastic_amb
    pure = np.zeros(n, bool)             # isotropic strain (c I, c R, tied values): the all_zero test is a coin toss by design
    if dpp.any():
        pure[idx] = res["amb_zero"]
    frac = float((amb & ~pure).sum()) / n
    report_margin(f"{tag}: decision-ambiguous particles outside isotropic strain (fraction)", frac, AMBIGUOUS_MAX,
                  count=int((amb & ~pure).sum()), pure_compression_ambiguous=int((amb & pure).sum()))
    assert frac <= AMBIGUOUS_MAX

    # stress: affine = -tau(F_out) * V0 * (4 / h^2) * dt, tau checked in fp64 from the F the kernel produced
    coeff = got.init_volume.astype(np.float64) * (4.0 / (H * H)) * DT
    tau_gpu = -T.mat(got.affine, dim) / coeff[:, None, None]
    lam, mu = got.lambda_.astype(np.float64), got.mu.astype(np.float64)
    assert np.array_equal(got.lambda_, ps.lambda_) and np.array_equal(got.mu, ps.mu)
    # (+ 2 u for the product tau * coeff and the fp32 coeff itself)
    fails = T.check_tau(f"{tag}: tau from affine", model, tau_gpu, F_out, lam, mu, T.svd_lapack(got.def_grad), c=T.C_TAU + 2)
    assert not fails, "\n".join(fails)
