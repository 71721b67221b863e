"""-m "not gpu": the host side of the device-side diagnostics — the elastic energy of tests/diag_truth.py against the ORACLE's
Kirchhoff stress (C2: what makes "elastic energy" the reference's energy and not a textbook variant), and the digest's two defining
properties (C3). C1, the ctypes twins of wgs_diagnostics and the WGS_SUM_* / WGS_DIAG_* values against the header as gcc sees it, is
tests/test_abi.py."""
import numpy as np
import pytest

import diag_truth as dt
from oracle import np_oracle


def _test_gradients(dim, rng, count=40):
    """Deformation gradients with singular values in [0.55, 1.6]: compressed, stretched, sheared and rotated, a few reflected."""
    out = []
    for i in range(count):
        q1, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
        q2, _ = np.linalg.qr(rng.normal(size=(dim, dim)))
        s = rng.uniform(0.55, 1.6, dim)
        F = q1 @ np.diag(s) @ q2.T
        if i % 5 != 4 and np.linalg.det(F) < 0:      # (every fifth keeps the sign chance gave it: det F < 0 is part of the domain)
            F[:, 0] *= -1.0
        out.append(F)
    out.append(np.eye(dim) + 1e-3 * rng.normal(size=(dim, dim)))      # near the rest state
    return np.array(out)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("model", [dt.MODEL_COROTATED, dt.MODEL_NEO_HOOKEAN])
def test_energy_derivative_is_the_oracle_stress(model, dim):
    """C2: central finite difference of diag_truth.psi along random unit directions H against the oracle's Kirchhoff stress:
    dPsi/dF : H = (tau F^-T) : H, tau from oracle/np_oracle.kirchoff_stress (the numpy twin of the C oracle).

    Tolerance, derived from the step eps = 1e-4 (|H|_F = 1):
      truncation  eps^2 / 6 * K3, K3 >= |third directional derivative|. ln det(F + tH) has third derivative 2 tr((F^-1 H)^3) <=
                  2 / s_min^3, (ln^2 J / 2)''' = 3 phi' phi'' + phi phi''' <= (3 sqrt(d) + 2 |ln J|) / s_min^3, ((J - 1)^2 / 2)''' =
                  3 J' J'' + (J - 1) J''' <= 3 sqrt(d) d (d - 1) s_max^(2d - 3) + 6 |J - 1|, and the rotation part of the corotated
                  energy, -2 mu tr sqrt(F^T F), has third derivatives bounded by 6 mu / (2 s_min)^2; for s in [0.55, 1.6] all of
                  them stay below K3 = 20 (lambda + mu) max(1, s_max)^d / min(1, s_min)^3;
      rounding    two evaluations of Psi, each a sum of pieces carrying at most 64 roundings of the largest piece (a 3 x 3
                  symmetric eigenvalue problem is the longest chain): 2 * 64 * 2^-53 * sum |pieces| / (2 eps);
      reflected F (det F < 0): the corotated energy has a kink where the two smallest singular values meet; directions that
                  cross it inside [-eps, eps] are not differentiable points and are left out (none in this seed)."""
    rng = np.random.default_rng(100 * dim + model)
    lam, mu, eps = 1.3, 0.7, 1.0e-4
    Fs = _test_gradients(dim, rng)
    if model == dt.MODEL_NEO_HOOKEAN:
        Fs = Fs[np.linalg.det(Fs) > 0]            # (the reference clamps J at 1e-10: below, the energy is flat and the stress is not its derivative)
    n = len(Fs)
    tau = np_oracle.kirchoff_stress(model, np.full(n, lam), np.full(n, mu), Fs)
    P = tau @ np.linalg.inv(Fs).transpose(0, 2, 1)
    worst = 0.0
    for _ in range(6):
        H = rng.normal(size=(n, dim, dim))
        H /= np.linalg.norm(H, axis=(1, 2))[:, None, None]
        fd = (dt.psi(model, Fs + eps * H, lam, mu) - dt.psi(model, Fs - eps * H, lam, mu)) / (2.0 * eps)
        exact = np.sum(P * H, axis=(1, 2))
        s = np.linalg.svd(Fs, compute_uv=False)
        k3 = 20.0 * (lam + mu) * np.maximum(1.0, s.max(1)) ** dim / np.minimum(1.0, s.min(1)) ** 3
        pieces = np.abs(dt.psi_parts(model, Fs, lam, mu)).sum(1)
        tol = eps * eps / 6.0 * k3 + 2.0 * 64.0 * 2.0 ** -53 * pieces / (2.0 * eps)
        err = np.abs(fd - exact)
        worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), (model, dim, float(np.max(err / tol)))
    assert worst > 0.0


@pytest.mark.parametrize("dim", [2, 3])
def test_digest_ignores_order_and_sees_every_bit(dim):
    """C3: a permutation of the rows leaves the digest alone; flipping ANY single bit of ANY hashed word (or of the id) of one
    particle changes both halves."""
    from wgsparkl_amd import scenes
    ps = scenes.random_cloud(12, dim=dim, seed=3)
    ids = np.arange(ps.n, dtype=np.uint32)
    words = dt.words_of(ps)
    assert words.shape[1] == 2 * dim + 2 * dim * dim + 5
    base = dt.digest_of_hashes(dt.particle_hashes(ids, words))
    assert base == dt.digest(ps)
    perm = np.random.default_rng(0).permutation(ps.n)
    assert dt.digest_of_hashes(dt.particle_hashes(ids[perm], words[perm])) == base
    assert dt.digest_of_hashes(dt.particle_hashes(ids, words[perm])) != base        # (the id is part of the hash)
    row = 5
    seen = {base}
    for w in range(-1, words.shape[1]):
        for bit in range(32):
            i2, w2 = ids.copy(), words.copy()
            if w < 0:
                i2[row] ^= np.uint32(1 << bit)
            else:
                w2[row, w] ^= np.uint32(1 << bit)
            got = dt.digest_of_hashes(dt.particle_hashes(i2, w2))
            assert got[0] != base[0] and got[1] != base[1], (w, bit)
            seen.add(got)
    assert len(seen) == 1 + 32 * (words.shape[1] + 1)                                # (and no two flips collide)


def test_fixed_sums_are_exact_on_a_dyadic_lattice():
    """The exponent rule and the integer sums of diag_truth itself, on values where everything is exact: the fixed sum times
    2^exponent IS the rational sum."""
    from fractions import Fraction
    from wgsparkl_amd import scenes
    rng = np.random.default_rng(5)
    ps = scenes.random_cloud(500, dim=3, seed=1)
    q = lambda shape, lo=-1024: (rng.integers(lo, 1025, shape) / 256.0).astype(np.float32)
    ps.pos[:], ps.vel[:], ps.mass[:] = q(ps.pos.shape, 400), q(ps.vel.shape), q(ps.mass.shape, 1)
    sums = dt.exact_sums(ps, 1.0, (0.0, -9.81, 0.0), energy=False)
    for name, col in (("mass", ps.mass[:, None]), ("momentum", ps.mass[:, None] * ps.vel), ("mass_moment", ps.mass[:, None] * ps.pos)):
        fixed, e = sums[name]
        for k in range(col.shape[1]):
            exact = sum(Fraction(float(m)) * (Fraction(float(c)) if name != "mass" else 1)
                        for m, c in zip(ps.mass, (ps.vel if name == "momentum" else ps.pos)[:, k]))
            assert Fraction(fixed[k]) * Fraction(2) ** e == exact
        assert abs(max(fixed, key=abs)) < 2 ** 62
