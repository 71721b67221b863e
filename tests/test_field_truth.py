"""-m "not gpu": the bounds of tests/field_truth.py are derived, not fitted. An honest fp32 numpy evaluation of the header's formulae
(field_truth.eval_fp32: LAPACK's fp32 SVD, numpy's fp32 log / expm1 / cbrt) stays inside every bound on every input set of
tests/test_gpu_fields.py that exists before a device ran — the states that test reads back after 24 / 30 substeps are represented by
their uploads —, and three wrong answers are each rejected. Nothing here runs the library."""
import numpy as np
import pytest

import devmath_truth as T
import field_truth as FT

SETS = {dim: FT.host_input_sets(dim) for dim in (3, 2)}


@pytest.mark.parametrize("dim,k", [(dim, k) for dim in (3, 2) for k in range(len(SETS[dim]))],
                         ids=[f"{dim}d-{name.replace(' ', '_')}" for dim in (3, 2) for name, _ in SETS[dim]])
def test_an_honest_fp32_evaluation_stays_inside_every_bound(dim, k):
    name, inp = SETS[dim][k]
    fails = FT.check_fields(f"fp32 numpy, {name} {dim}d", inp, FT.eval_fp32(inp))
    assert not fails, "\n".join(fails[:12])


def _well_conditioned(dim, model):
    """the catalogue's well-conditioned family with per-particle material: every bound is far below 1e-3 of the stress there"""
    ps = FT.catalogue_particles(dim, model, True)
    fam = T.catalogue(dim, seed=5)["well_conditioned"]
    ps = FT.Inputs.of(ps, model)
    n = len(fam)
    return FT.Inputs(fam, ps.lam[:n], ps.mu[:n], ps.model[:n], ps.gamma)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("model", [0, 1])
def test_the_stress_of_the_other_model_is_rejected(dim, model):
    inp = _well_conditioned(dim, model)
    assert not FT.check_fields("right model", inp, FT.eval_fp32(inp))
    other = FT.eval_fp32(FT.Inputs(inp.def_grad, inp.lam, inp.mu, 1 - inp.model, inp.gamma))
    other.model = inp.model.astype(np.uint32)                      # (the label alone would give it away)
    fails = FT.check_fields("other model", inp, other)
    assert any("tau normwise" in f for f in fails), fails


@pytest.mark.parametrize("dim", [3, 2])
def test_records_permuted_by_one_slot_are_rejected(dim):
    inp = _well_conditioned(dim, 0)
    good = FT.eval_fp32(inp)
    for f in ("stress", "mean_stress", "von_mises", "volume_ratio", "stretch", "model"):
        setattr(good, f, np.roll(getattr(good, f), 1, axis=0))
    fails = FT.check_fields("rolled by one", inp, good)
    for what in ("tau normwise", "stretch |s - s64|", "volume_ratio"):
        assert any(what in f for f in fails), (what, fails)
    assert not any("mean_stress" in f or "von_mises" in f for f in fails), "the invariants still belong to their own record's stress"


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("model", [0, 1])
def test_a_transposed_stress_is_rejected(dim, model):
    """tau is symmetric, so a transposition shows only on its non-symmetric part: the answer carries a strictly upper-triangular
    perturbation of 1e-3 |tau| and is then transposed, which a reader that mixes up rows and columns would do to the kernel's rounding
    asymmetry writ large. Both are outside the bound."""
    inp = _well_conditioned(dim, model)
    good = FT.eval_fp32(inp)
    E = np.triu(np.ones((dim, dim)), 1)
    E = E / np.linalg.norm(E)
    bad = FT.eval_fp32(inp)
    bad.stress = np.transpose(good.stress + (1e-3 * np.linalg.norm(good.stress, axis=(1, 2)))[:, None, None] * E, (0, 2, 1)).astype(np.float32)
    fails = FT.check_fields("transposed", inp, bad)
    assert any("tau normwise" in f for f in fails), fails


def test_the_fluid_bound_vanishes_at_rest_and_grows_with_the_exponent():
    J = np.array([1.0, 1.0 + 2.0 ** -23, 0.5, 2.0])
    b = FT.fluid_stress_bound(J, np.full(4, 1.0e6), 7.0)
    assert b[0] == 0.0 and 0.0 < b[1] < 1e-3 and b[2] > b[3] > 0.0


def test_the_invariants_survive_a_stress_without_an_fp32_square():
    """|tau| = 1e25 (an inverted element under lambda 1e5 at scale 1e3): the sum of squares is scaled by a power of two"""
    t = np.zeros((2, 3, 3), np.float32)
    t[0] = np.diag([1e25, -2e25, 3e25])
    t[1] = np.diag([1e-25, -2e-25, 3e-25])
    mean, vm = FT.invariants32(t)
    fails = []
    FT.check_invariants("extreme", t, mean, vm, fails)
    assert not fails and np.isfinite(vm).all() and (vm > 0).all()
