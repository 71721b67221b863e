"""fp64 truth and a-priori bounds for the Lagrangian field output (include/wgsparkl_hip.h "Lagrangian field output";
wgsparkl_amd/csrc/kernels_fields.h): the Kirchhoff stress, its two invariants, the volume ratio and the stretches of a particle's
stored state, from the SAME fp32 def_grad / lambda / mu the kernel sees.

TEST INFRASTRUCTURE ONLY. The stress and singular-value truth and their bounds are those of tests/devmath_truth.py (check_tau,
tau_scales, the singular-value bound and the sign rule of check_svd), the fluid's is tests/fluid_truth.py kirchhoff with G = 0;
neither file is changed. Every bound is C * u * scale with u = 2^-24 and is reported through helpers.report_margin
(measured / bound, so 1.0 is the edge). Shared by tests/test_field_truth.py (an honest fp32 numpy evaluation must stay inside the
bounds, three wrong answers must not) and tests/test_gpu_fields.py (the device)."""
import types
from typing import NamedTuple

import numpy as np

import devmath_truth as T
import fluid_truth as ft
from helpers import report_margin

U32 = T.U32
C_DET = 8        # volume ratio: 6 triple products of 2 roundings each plus 5 additions
C_VM = 32        # von Mises stress, absolute in |stress|_F (derivation at the check)
C_ISO = 4        # the fluid's isotropic stretch: one cbrt / sqrt of J
MODEL_FLUID = 2


class Inputs(NamedTuple):
    """what the kernel sees of n particles"""
    def_grad: np.ndarray   # [n, D*D] fp32, column-major (fluid: diag(J, 1[, 1]))
    lam: np.ndarray        # [n] fp32
    mu: np.ndarray         # [n] fp32
    model: np.ndarray      # [n] the model of every particle: 0, 1 or 2
    gamma: float           # the Tait exponent of the data

    @classmethod
    def of(cls, particles, model, gamma=7.0):
        """from a ParticleSet (the upload, or read_particles() of the moment) and the data's model or its per-particle table"""
        n = particles.n
        m = np.full(n, model, np.int64) if np.ndim(model) == 0 else np.asarray(model, np.int64).reshape(n)
        return cls(np.asarray(particles.def_grad, np.float32), np.asarray(particles.lambda_, np.float32),
                   np.asarray(particles.mu, np.float32), m, float(gamma))

    def take(self, idx):
        return Inputs(self.def_grad[idx], self.lam[idx], self.mu[idx], self.model[idx], self.gamma)

    @property
    def dim(self):
        return int(round(np.sqrt(self.def_grad.shape[1])))


def _bound(fails, tag, name, err, b, what=None):
    err, b = np.asarray(err, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if not err.size:
        return
    r = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(r), np.inf, r)
    w = int(np.argmax(r))
    bad = ~(err <= b)
    report_margin(f"{tag}: {name}", float(err[w]), float(b[w]), n=int(err.size), failures=int(bad.sum()))
    if bad.any():
        i = int(np.argmax(bad))
        fails.append(f"{tag}: {name}: {int(bad.sum())}/{err.size} over the bound (first #{i if what is None else int(what[i])}: "
                     f"{err[i]:.3e} > {b[i]:.3e})")


def fluid_stress_bound(J, lam, gamma):
    """C_TAU u (|lambda| / gamma) Jc (|Jc^-gamma - 1| + gamma |ln Jc| Jc^-gamma): the first term is the relative error of the
    products and of expm1 itself, the second the absolute error of its argument -gamma ln Jc (a few u of its size) carried through the
    expm1, whose derivative is exp(-gamma ln Jc) = Jc^-gamma."""
    J, lam = np.asarray(J, np.float64), np.asarray(lam, np.float64)
    Jc = np.maximum(J, ft.J_MIN)
    pw = Jc ** -gamma
    return T.C_TAU * U32 * (np.abs(lam) / gamma) * Jc * (np.abs(np.expm1(-gamma * np.log(Jc))) + gamma * np.abs(np.log(Jc)) * pw)


def check_stretch(tag, S, svd64, fails):
    """The singular-value bound and the sign rule of devmath_truth.check_svd, for the values alone: C_SV u s_max on the sorted |s|;
    exactly one negative value iff det F < 0, on the smallest |s|, decided only where |s_min| > 2 x that bound."""
    st = svd64[1]
    abs_t, smax, _ = T.sv_stats(st)
    S = np.asarray(S, np.float64)
    a = np.sort(np.abs(S), 1)[:, ::-1]
    sv_err = T.C_SV * U32 * smax
    _bound(fails, tag, "stretch |s - s64| (scale s_max)", np.abs(a - abs_t).max(1), sv_err)
    clear = abs_t[:, -1] > 2.0 * sv_err
    neg_t = st.min(1) < 0
    nneg = (S < 0).sum(1)
    wrong = clear & (nneg != np.where(neg_t, 1, 0))
    on_small = np.abs(np.where(S < 0, S, np.inf)).min(1)
    wrong |= clear & neg_t & ~(on_small <= np.abs(S).min(1) + sv_err)
    report_margin(f"{tag}: stretch sign convention violations", float(wrong.sum()), 0.0, checked=int(clear.sum()))
    if wrong.any():
        i = int(np.argmax(wrong))
        fails.append(f"{tag}: stretch sign convention wrong for {int(wrong.sum())} of {int(clear.sum())} (first #{i}: s = {S[i]}, truth {st[i]})")


def check_invariants(tag, stress32, mean, von_mises, fails):
    """mean_stress and von_mises against fp64 values of the record's OWN fp32 stress [n, D, D].

    mean: D - 1 additions and one division of numbers no larger than sum |tau_kk|: (D + 1) u sum |tau_kk| / D.

    von Mises, ABSOLUTE in |stress|_F because the deviator cancels (an isotropic stress has vm64 = 0 and a computed one of the size of
    the mean's error). Per entry of the deviator: off the diagonal it is the stored word, exact; on it dev = fl(tau_kk - mean) is off by
    the mean's error e_m <= (D + 1) u sum |tau_kk| / D <= (D + 1) u |tau|_F / sqrt(D) plus u |dev|, so the deviator as a vector of D^2
    entries is off by sqrt(D) e_m + u |dev|_F <= (D + 2) u |tau|_F in the 2-norm. The sum q of D^2 squares (all positive, so its
    D^2 - 1 additions and D^2 products add (D^2 + 1) u q relative; the kernel scales by a power of two first, which is exact):
    delta sqrt(q) = delta q / (2 sqrt q) <= |delta dev|_2 + (D^2 + 1) / 2 u sqrt(q). The product with 3/2 and the square root add 1.5 u
    relative. With sqrt(q) = |dev|_F <= |tau|_F and the factor sqrt(3/2): sqrt(3/2) (D + 2 + (D^2 + 1) / 2 + 1.5) u |tau|_F =
    14.1 u |tau|_F in 3D, 9.8 u in 2D. C_VM = 32 holds both with a factor 2."""
    t = np.asarray(stress32, np.float32).astype(np.float64)
    d = t.shape[1]
    diag = np.diagonal(t, axis1=1, axis2=2)
    mean64 = diag.sum(1) / d
    _bound(fails, tag, "mean_stress (scale sum |tau_kk| / D)", np.abs(np.asarray(mean, np.float64) - mean64),
           (d + 1) * U32 * np.abs(diag).sum(1) / d)
    dev = t - mean64[:, None, None] * np.eye(d)
    vm64 = np.sqrt(1.5 * (dev * dev).sum((1, 2)))
    _bound(fails, tag, "von_mises (absolute, scale |stress|_F)", np.abs(np.asarray(von_mises, np.float64) - vm64),
           C_VM * U32 * np.linalg.norm(t, axis=(1, 2)))


def check_fields(tag, inp, fields):
    """Every field of `fields` (a wgsparkl_amd.pipeline.ParticleFields, or anything with its arrays) against the truth of `inp`.
    Returns the list of failures (empty = pass); every bound is reported."""
    d = inp.dim
    fails = []
    n = len(inp.lam)
    stress = np.asarray(fields.stress)
    assert stress.shape == (n, d, d) and np.asarray(fields.stretch).shape == (n, d), (stress.shape, n, d)
    if not np.array_equal(np.asarray(fields.model).astype(np.int64), inp.model):
        w = np.nonzero(np.asarray(fields.model).astype(np.int64) != inp.model)[0]
        fails.append(f"{tag}: model differs for {len(w)} particles (first #{int(w[0])}: {int(fields.model[w[0]])}, expected {int(inp.model[w[0]])})")
    for model in (0, 1):
        idx = np.nonzero(inp.model == model)[0]
        if not len(idx):
            continue
        sub = inp.take(idx)
        F = T.mat(sub.def_grad, d)
        svd64 = T.svd_lapack(sub.def_grad)
        name = f"{tag} [{'corotated' if model == 0 else 'neo-Hookean'}]"
        fails += T.check_tau(name, model, stress[idx].astype(np.float64), F, sub.lam.astype(np.float64), sub.mu.astype(np.float64), svd64)
        check_stretch(name, fields.stretch[idx], svd64, fails)
        # |J - det64 F| <= 8 u |F|_F^D: the sum of the |products| of a determinant is at most the product of the column norms, at
        # most |F|_F^D; every product carries 2 roundings and the 5 additions (2D: one) one each
        _bound(fails, name, "volume_ratio |J - det F| (scale |F|^D)", np.abs(fields.volume_ratio[idx].astype(np.float64) - np.linalg.det(F)),
               C_DET * U32 * np.linalg.norm(F, axis=(1, 2)) ** d, idx)
    idx = np.nonzero(inp.model == MODEL_FLUID)[0]
    if len(idx):
        sub = inp.take(idx)
        name = f"{tag} [fluid]"
        J = sub.def_grad[:, 0].astype(np.float64)
        if not np.array_equal(fields.volume_ratio[idx], sub.def_grad[:, 0]):
            fails.append(f"{name}: volume_ratio is not def_grad[0] bit for bit")
        t64 = ft.kirchhoff(J, np.zeros((len(idx), d, d)), sub.lam.astype(np.float64), sub.mu.astype(np.float64), sub.gamma)
        _bound(fails, name, "fluid tau normwise", np.linalg.norm(stress[idx].astype(np.float64) - t64, axis=(1, 2)),
               fluid_stress_bound(J, sub.lam, sub.gamma), idx)
        with np.errstate(invalid="ignore"):
            iso = np.cbrt(J) if d == 3 else np.sqrt(J)
        _bound(fails, name, "fluid stretch |s - J^(1/D)| (scale J^(1/D))", np.abs(fields.stretch[idx].astype(np.float64) - iso[:, None]).max(1),
               C_ISO * U32 * np.abs(iso), idx)
    check_invariants(tag, stress, fields.mean_stress, fields.von_mises, fails)
    return fails


# ------------------------------------------------------------------------------------------------ an honest fp32 evaluation
def _svd32(F):
    """fp32 LAPACK SVD in the shipped convention (devmath_truth.svd_lapack, in fp32)"""
    U, s, Vt = np.linalg.svd(F.astype(np.float32))
    U, s, V = U.copy(), s.copy(), np.transpose(Vt, (0, 2, 1)).copy()
    fu, fv = np.linalg.det(U.astype(np.float64)) < 0, np.linalg.det(V.astype(np.float64)) < 0
    U[fu, :, -1] *= np.float32(-1.0)
    V[fv, :, -1] *= np.float32(-1.0)
    s[fu != fv, -1] *= np.float32(-1.0)
    return U, s, V


def _det32(F):
    f = np.float32
    if F.shape[1] == 2:
        return (F[:, 0, 0] * F[:, 1, 1] - F[:, 0, 1] * F[:, 1, 0]).astype(f)
    m = lambda r, c: F[:, r, c]
    return (m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0))
            + m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0))).astype(f)


def invariants32(stress):
    """mean_stress and von_mises as the header states them, in fp32: the diagonal summed k = 0 .. D-1 and divided by D; the deviator
    scaled by the power of two of its largest entry (exact), squared and summed in storage order (column-major), times 3/2, square
    root, scaled back."""
    f = np.float32
    t = np.asarray(stress, f)
    n, d, _ = t.shape
    tr = t[:, 0, 0].copy()
    for k in range(1, d):
        tr = (tr + t[:, k, k]).astype(f)
    mean = (tr / f(d)).astype(f)
    dev = t.copy()
    for k in range(d):
        dev[:, k, k] = (t[:, k, k] - mean).astype(f)
    m = np.abs(dev).max((1, 2))
    with np.errstate(all="ignore"):
        _, e = np.frexp(m)
        e = np.where(np.isfinite(m), e, 0).astype(np.int32)
        q = np.zeros(n, f)
        for c in range(d):
            for r in range(d):
                x = np.ldexp(dev[:, r, c], -e).astype(f)
                q = (q + (x * x).astype(f)).astype(f)
        vm = np.ldexp(np.sqrt((f(1.5) * q).astype(f)).astype(f), e).astype(f)
    return mean, vm


def eval_fp32(inp):
    """The formulae of the header evaluated in fp32 numpy (LAPACK's fp32 SVD, numpy's fp32 log / expm1 / cbrt): what an honest
    implementation in the step's precision computes. Nothing here is tuned: it has to stay inside every bound of check_fields."""
    f = np.float32
    d = inp.dim
    n = len(inp.lam)
    F = T.mat(inp.def_grad, d).astype(f)
    lam, mu = inp.lam.astype(f), inp.mu.astype(f)
    eye = np.eye(d, dtype=f)
    stress = np.zeros((n, d, d), f)
    stretch = np.zeros((n, d), f)
    J = np.zeros(n, f)
    with np.errstate(all="ignore"):
        solid = inp.model != MODEL_FLUID
        if solid.any():
            U, s, V = _svd32(F[solid])
            stretch[solid] = s
            J[solid] = _det32(F[solid])
        m0 = inp.model == 0
        if m0.any():
            U, s, V = _svd32(F[m0])
            j = np.prod(s, 1, dtype=f)
            rec = ((U * (s - f(1.0))[:, None, :]) @ np.transpose(V, (0, 2, 1))).astype(f)            # F - R
            t = (rec @ np.transpose(F[m0], (0, 2, 1))).astype(f) * (f(2.0) * mu[m0])[:, None, None]
            stress[m0] = (t + (lam[m0] * (j - f(1.0)) * j)[:, None, None] * eye).astype(f)
        m1 = inp.model == 1
        if m1.any():
            j = np.maximum(_det32(F[m1]), f(T.NH_CLAMP))
            fft = (F[m1] @ np.transpose(F[m1], (0, 2, 1))).astype(f)
            stress[m1] = (mu[m1][:, None, None] * fft + (lam[m1] * np.log(j) - mu[m1])[:, None, None] * eye).astype(f)
        m2 = inp.model == MODEL_FLUID
        if m2.any():
            g = f(inp.gamma)
            j = F[m2][:, 0, 0]
            jc = np.maximum(j, f(ft.J_MIN))
            p = ((lam[m2] / g) * np.expm1((-g * np.log(jc)).astype(f)).astype(f)).astype(f)
            stress[m2] = (-(jc * p))[:, None, None] * eye
            J[m2] = j
            stretch[m2] = (np.cbrt(j) if d == 3 else np.sqrt(j)).astype(f)[:, None]
        mean, vm = invariants32(stress)
    return types.SimpleNamespace(stress=stress, mean_stress=mean, von_mises=vm, volume_ratio=J, stretch=stretch,
                                 model=inp.model.astype(np.uint32))


# ------------------------------------------------------------------------------------------------ the input sets of the GPU test
H = 1.0
DT = 1.0e-3
TAILS = (1, 63, 257, 4097)


def catalogue_particles(dim, model, per_particle, n=None, seed=0):
    """n (default 3000 in 3D, 2000 in 2D) particles at random positions whose def_grad walks through devmath_truth.catalogue — every
    family first, then random draws —, uniform or per-particle lambda / mu / mass as tests/test_gpu_constitutive.py sets them."""
    from wgsparkl_amd.models import ElasticCoefficients, ParticlePhase
    from wgsparkl_amd.solver import ParticleSet
    rng = np.random.default_rng(4200 + 10 * seed + dim)
    n = (3000 if dim == 3 else 2000) if n is None else n
    pos = rng.uniform(2.0, 10.0, (n, dim)).astype(np.float32)
    ps = ParticleSet.uniform(pos, H / 4.0, 10.0, ElasticCoefficients.from_young_modulus(1e5, 0.3), phase=ParticlePhase(1.0, -1.0))
    F = np.concatenate(list(T.catalogue(dim, seed=5 + seed).values()))
    idx = np.concatenate([np.arange(len(F)), rng.integers(0, len(F), max(0, n - len(F)))])[:n]
    if n < len(F):
        idx = rng.permutation(len(F))[:n]
    ps.def_grad[:] = F[idx]
    if per_particle:
        ps.lambda_[:] = (ps.lambda_ * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        ps.mu[:] = (ps.mu * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        ps.mass[:] = (ps.mass * rng.uniform(0.5, 1.5, n)).astype(np.float32)
        if model == 1:
            ps.mu[::5] = 0.0
    return ps


def fluid_particles(dim, n=None, seed=0):
    """catalogue_particles with def_grad = diag(J, 1[, 1]): J from strong compression to strong expansion, J = 1 exactly and its two
    fp32 neighbours; lambda = bulk modulus, mu = viscosity per particle. (Nothing near the clamp 1e-10: below J = 3e-6 the fp32
    power Jc^-7 is infinite, in the step as here, and no bound of the form C u scale says anything about it.)"""
    ps = catalogue_particles(dim, 0, True, n, seed + 50)
    rng = np.random.default_rng(77 + seed + dim)
    n = ps.n
    J = np.exp(rng.uniform(np.log(0.5), np.log(2.0), n))
    special = np.array([1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 1e-3, 0.05, 30.0])
    J[:min(n, len(special))] = special[:min(n, len(special))]
    ps.def_grad[:] = ft.fluid_def_grad(J.astype(np.float32), dim)
    ps.lambda_[:] = (1.0e6 * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    ps.mu[:] = rng.uniform(0.0, 5.0, n).astype(np.float32)
    return ps


def mixed_particles(dim, n=None, seed=0):
    """(particles, table): catalogue_particles with one of the three models per particle; the fluid ones carry diag(J, 1[, 1])"""
    ps = catalogue_particles(dim, 1, True, n, seed + 20)
    fl = fluid_particles(dim, ps.n, seed + 20)
    table = (np.arange(ps.n) * 7 % 3).astype(np.uint8)
    m2 = table == MODEL_FLUID
    ps.def_grad[m2] = fl.def_grad[m2]
    ps.lambda_[m2] = fl.lambda_[m2]
    ps.mu[m2] = fl.mu[m2]
    return ps, table


def host_input_sets(dim):
    """(name, Inputs) of every input set of tests/test_gpu_fields.py that exists before anything ran on a device: the catalogue cases,
    the tail sizes, the fluid and mixed sets, the Drucker-Prager catalogue of the zero-momentum construction, and the uploads of the
    scenes whose LATER states (after 24 / 30 substeps) the device test reads back."""
    out = []
    for model in (0, 1):
        for pp in (False, True):
            out.append((f"catalogue model {model} {'per-particle' if pp else 'uniform'}", Inputs.of(catalogue_particles(dim, model, pp), model)))
    for n in TAILS:
        out.append((f"tail n={n}", Inputs.of(catalogue_particles(dim, n % 2, True, n=n, seed=n), n % 2)))
    out.append(("fluid", Inputs.of(fluid_particles(dim), MODEL_FLUID)))
    ps, table = mixed_particles(dim)
    out.append(("mixed table", Inputs.of(ps, table)))
    rng = np.random.default_rng(31 + dim)
    Fdp = np.concatenate(list(T.dp_catalogue(dim, rng).values()))
    ps = catalogue_particles(dim, 0, True, n=len(Fdp), seed=9)
    ps.def_grad[:] = Fdp
    out.append(("Drucker-Prager catalogue", Inputs.of(ps, 0)))
    out.append(("cloud upload", Inputs.of(flying_cloud(dim)["particles"], 0)))
    sc = small_block_in_fluid(dim)
    out.append(("block_in_fluid upload", Inputs.of(sc["particles"], sc["models"], sc["fluid_gamma"])))
    if dim == 3:
        sc = small_tait_block()
        out.append(("tait_fluid_block upload", Inputs.of(sc["particles"], MODEL_FLUID, sc["fluid_gamma"])))
    return out


def flying_cloud(dim):
    """gpu_common.cloud_scene flying through the grid: the sort moves particles every substep"""
    from gpu_common import cloud_scene
    sc = cloud_scene(n=6000 if dim == 3 else 4000, dim=dim, seed=11)
    sc["particles"].vel[:] += np.array([60.0, 25.0, -40.0][:dim], np.float32)     # 1.8 cells along x in 30 substeps
    return sc


def small_block_in_fluid(dim):
    from wgsparkl_amd import scenes
    return scenes.block_in_fluid(dim=dim, tank=(12, 8, 8) if dim == 3 else (24, 12), block=4, gap=0.1, drop_speed=6.0)


def small_tait_block():
    from wgsparkl_amd import scenes
    sc = scenes.tait_fluid_block(nx=16, ny=12, nz=12, bulk_modulus=2.0e5, viscosity=2.0, grid_capacity=2048)
    ps = sc["particles"]            # (the block hangs above the floor: in free fall J would stay 1, so it starts converging on its centre)
    ps.vel[:] = (-3.0 * (ps.pos - ps.pos.mean(0))).astype(np.float32)
    return sc
