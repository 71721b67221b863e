"""The shipped device math (wgsparkl_amd/csrc/device_math.h) one lane per matrix, against fp64 truth of the same fp32 inputs
(tests/devmath_truth.py): the one-sided Jacobi SVD, the corotated and neo-Hookean Kirchhoff stresses and the Drucker-Prager
projection, over a catalogue of hard deformations (inverted, clustered, rank-deficient, badly conditioned, structured,
far from F = I in scale) and F values recorded from real runs. Checked per matrix, with a-priori bounds in units of
u = 2^-24; also that a lane's result depends on its own matrix only (the sweep loop leaves on a vote of the whole wave).

The probe (tests/hip/devmath_probe.hip) is compiled here with the flags of wgsparkl_amd/csrc/build.sh, so its rounding is
the shipped rounding; the compile alone also runs without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import devmath_truth as T
from helpers import oracle, report_margin
from oracle import np_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wgsparkl_amd", "csrc")
PROBE_SRC = os.path.join(ROOT, "tests", "hip", "devmath_probe.hip")
# csrc/build.sh's flags (the fp rounding of the product), for one dimension
PROBE_FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-fno-fast-math", "-ffp-contract=on"]


def compile_probe(dim, outdir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(str(outdir), f"devmath_probe{dim}d.so")
    r = subprocess.run([hipcc, *PROBE_FLAGS, f"-DWGS_DIM={dim}", "-I", CSRC, PROBE_SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, f"probe compile failed (dim {dim}):\n{r.stderr[-4000:]}"
    return out


class Probe:
    def __init__(self, path, dim):
        self.lib = C.CDLL(path)
        self.dim = dim
        assert self.lib.probe_dim() == dim
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        self.lib.probe_svd.argtypes = [fp, C.c_int, fp, fp, fp]
        self.lib.probe_stress.argtypes = [C.c_int, fp, fp, fp, C.c_int, fp]
        self.lib.probe_dp.argtypes = [fp, fp, fp, C.c_int, ip, fp, fp]

    @staticmethod
    def _p(a, t=C.c_float):
        return a.ctypes.data_as(C.POINTER(t))

    def svd(self, F32):
        F = np.ascontiguousarray(F32, np.float32)
        n, d = len(F), self.dim
        U, S, V = np.zeros((n, d * d), np.float32), np.zeros((n, d), np.float32), np.zeros((n, d * d), np.float32)
        rc = self.lib.probe_svd(self._p(F), n, self._p(U), self._p(S), self._p(V))
        assert rc == 0, f"probe_svd: hip error {rc}"
        return U, S, V

    def stress(self, model, lam, mu, F32):
        F = np.ascontiguousarray(F32, np.float32)
        lam, mu = np.ascontiguousarray(lam, np.float32), np.ascontiguousarray(mu, np.float32)
        tau = np.zeros_like(F)
        rc = self.lib.probe_stress(int(model), self._p(lam), self._p(mu), self._p(F), len(F), self._p(tau))
        assert rc == 0, f"probe_stress: hip error {rc}"
        return tau

    def dp(self, dp, state, F32):
        F = np.ascontiguousarray(F32, np.float32)
        dp, state = np.ascontiguousarray(dp, np.float32), np.ascontiguousarray(state, np.float32)
        n = len(F)
        ch, so, Fo = np.zeros(n, np.int32), np.zeros((n, 3), np.float32), np.zeros_like(F)
        rc = self.lib.probe_dp(self._p(dp), self._p(state), self._p(F), n, self._p(ch, C.c_int), self._p(so), self._p(Fo))
        assert rc == 0, f"probe_dp: hip error {rc}"
        return ch.astype(bool), so, Fo


@pytest.fixture(scope="session")
def probes(tmp_path_factory):
    d = tmp_path_factory.mktemp("devmath_probe")
    return {dim: Probe(compile_probe(dim, d), dim) for dim in (2, 3)}


def test_probe_compiles(tmp_path):
    """No GPU needed: the probe still compiles against the current device_math.h, in both dimensions."""
    for dim in (2, 3):
        assert os.path.getsize(compile_probe(dim, tmp_path)) > 0


def test_catalogue_and_truths_agree():
    """No GPU needed: the catalogue holds what it says (inverted, tied, rank-deficient, near the cutoff), and the fp64 truth
    of devmath_truth agrees to fp64 round-off with the C oracle's Jacobi (SVD, stresses) and with oracle/np_oracle.py
    (stresses, and the Drucker-Prager branch it takes)."""
    for dim in (2, 3):
        cat = T.catalogue(dim)
        orc = oracle(dim, np.float64)
        for fam, F32 in cat.items():
            U, s, V = T.svd_lapack(F32)
            Uc, sc, Vc = T.svd_c_oracle(orc, F32)
            a, smax, _ = T.sv_stats(s)
            ac, _, _ = T.sv_stats(sc)
            assert np.all(np.abs(a - ac).max(1) <= 1e-12 * np.maximum(smax, 1e-300) + 1e-300), fam
            F = T.mat(F32, dim)
            assert np.all(np.linalg.norm(Uc @ (sc[:, :, None] * np.transpose(Vc, (0, 2, 1))) - F, axis=(1, 2)) <=
                          1e-12 * np.linalg.norm(F, axis=(1, 2)) + 1e-300), fam
            # neo-Hookean through both routes; corotated where it is unique
            lam = np.full(len(F32), 3.0)
            mu = np.full(len(F32), 2.0)
            for model in (0, 1):
                t64 = T.tau_corotated64(F, lam, mu, U, s) if model == 0 else T.tau_neo_hookean64(F, lam, mu)
                tc = np.stack([T.mat(orc.kirchoff_stress(model, 3.0, 2.0, f.astype(np.float64))[None], dim)[0] for f in F32])
                ok = T.tau_unique(s) if model == 0 else np.ones(len(F32), bool)
                scale = T.tau_scales(model, F, lam, mu, s)
                assert np.all(np.linalg.norm(tc - t64, axis=(1, 2))[ok] <= 1e-10 * scale[ok]), (fam, model)
            # the stress truth is the one oracle/np_oracle.py computes (LAPACK SVD, its own convention code)
            for model in (0, 1):
                t64 = T.tau_corotated64(F, lam, mu, U, s) if model == 0 else T.tau_neo_hookean64(F, lam, mu)
                tn = np_oracle.kirchoff_stress(model, lam, mu, F)
                ok = T.tau_unique(s) if model == 0 else np.ones(len(F32), bool)
                assert np.all(np.linalg.norm(tn - t64, axis=(1, 2))[ok] <= 1e-10 * T.tau_scales(model, F, lam, mu, s)[ok]), (fam, model)
        # the Drucker-Prager truth: every branch's outcome (devmath_truth.dp_outcomes64) — the one np_oracle takes agrees
        from wgsparkl_amd.models import DruckerPrager
        for fam, F32 in T.dp_catalogue(dim, np.random.default_rng(dim)).items():
            n = len(F32)
            dp = np.tile(DruckerPrager.new(1e6, 0.25).as_array().astype(np.float64), (n, 1))
            state = np.tile(np.array([1.0, 1.0, 0.0]), (n, 1))
            F = T.mat(F32, dim)
            res = T.dp_outcomes64(dp, state, F, T.svd_lapack(F32))
            Fn, sn = np_oracle.drucker_prager_project(dp, state, F)
            clear = np.array([len(a) == 1 for a in T.dp_allowed(res)])
            for br in ("A", "B", "N"):
                sel = clear & (res["branch"] == br)
                assert np.allclose(Fn[sel], res["out"][br]["F"][sel], rtol=1e-9, atol=1e-9), (fam, br)
                assert np.allclose(sn[sel], res["out"][br]["state"][sel], rtol=1e-9, atol=1e-9), (fam, br)
        assert (np.linalg.det(T.mat(cat["inverted_distinct"], dim)) < 0).all()
        assert (np.linalg.det(T.mat(cat["inverted_tied"], dim)) < 0).all()
        a, smax, _ = T.sv_stats(T.svd_lapack(cat["near_cutoff"])[1])
        r = a[:, -1] / smax
        assert (r < T.CUTOFF).any() and (r > T.CUTOFF).any()


def _recorded_F(dim):
    """F values of real runs, recorded at test time (nothing committed): a few hundred substeps of a sand column
    (the C3 workload's material at test size, Drucker-Prager) and a stretched elastic cube, through the product's kernels."""
    from helpers import run_gpu
    from wgsparkl_amd import scenes
    from wgsparkl_amd.solver import SimulationParams
    out = []
    if dim == 3:
        sc = scenes.sand_column(nx=8, ny=16, nz=8)
        sc["params"] = SimulationParams(gravity=(0.0, -9.81, 0.0), dt=sc["params"].dt)
        data = run_gpu(sc, 240)
        out.append(data.read_particles().def_grad)
        sc = scenes.neo_hookean_cube(n_side=8)
        ps = sc["particles"]
        c = ps.pos.mean(0)
        ps.vel[:] = ((ps.pos - c) * np.array([6.0, -3.0, 1.0])).astype(np.float32)   # stretched along x, squeezed along y
        sc["params"] = SimulationParams(gravity=(0.0, 0.0, 0.0), dt=sc["params"].dt)
        data = run_gpu(sc, 200)
        out.append(data.read_particles().def_grad)
    else:
        sc = scenes.elastic_block_2d(nx=24, ny=24, with_floor=True)
        data = run_gpu(sc, 300)
        out.append(data.read_particles().def_grad)
    F = np.concatenate(out).astype(np.float32)
    assert np.isfinite(F).all()
    return F


def _families(dim, with_recorded):
    cat = dict(T.catalogue(dim))
    if with_recorded:
        cat["recorded_runs"] = _recorded_F(dim)
    return cat


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 2])
def test_svd_against_fp64_per_matrix(probes, hip_libs, dim):
    fails = []
    for fam, F32 in _families(dim, True).items():
        U, S, V = probes[dim].svd(F32)
        fails += T.check_svd(f"svd{dim}d {fam}", F32, T.mat(U, dim), S.astype(np.float64), T.mat(V, dim), T.svd_lapack(F32))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("model", [0, 1], ids=["corotated", "neo_hookean"])
def test_stress_against_fp64_per_matrix(probes, hip_libs, dim, model):
    """tau per matrix (devmath_truth.check_tau). Corotated: normwise with scale 2 mu |F| (|F| + 1) + |lambda| (|J| + dJ)
    (|J| + 1) times s_max / s_kept_min where tau is unique, and its trace — which depends on the singular values only —
    without that factor on every matrix. Neo-Hookean: normwise, including mu = 0 (the C5 "fluid") and the det <= 1e-10
    clamp, held to u where the clamp has decided (inverted elements: the pressure is lambda log 1e-10)."""
    rng = np.random.default_rng(77 + dim + 10 * model)
    fails = []
    for fam, F32 in _families(dim, False).items():
        n = len(F32)
        lam = rng.uniform(0.0, 5.0, n).astype(np.float32)
        mu = rng.uniform(0.0, 3.0, n).astype(np.float32)
        mu[::4] = 0.0                                    # pressure only
        tau = T.mat(probes[dim].stress(model, lam, mu, F32), dim)
        fails += T.check_tau(f"tau{dim}d model {model} {fam}", model, tau, T.mat(F32, dim), lam.astype(np.float64),
                             mu.astype(np.float64), T.svd_lapack(F32))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 2])
def test_drucker_prager_against_fp64_per_matrix(probes, hip_libs, dim):
    """changed flag, plastic state and projected F per matrix. A particle whose fp64 decision quantities (trace ≷ 0, the
    exact-equality all_zero of pure compression, gamma ≤ 0) lie within the fp32 band of the threshold may take either side;
    its result must then be one of the legitimate outcomes, each computed in fp64 from the same input. Pure compression
    F = c I is the standing example: log c summed d times and divided by d is not always log c in fp32, so the kernel may
    keep F (the cone branch finds gamma ≤ 0) or project to the tip. Inverted F: log of a negative singular value is NaN in
    the reference too — out of scope, only NaN-ness is compared with the C oracle."""
    from wgsparkl_amd.models import DruckerPrager
    rng = np.random.default_rng(303 + dim)
    base = DruckerPrager.new(1e6, 0.25).as_array()
    orc = oracle(dim, np.float64)
    fails, n_amb, n_tot = [], 0, 0
    for fam, F32 in T.dp_catalogue(dim, rng).items():
        n = len(F32)
        dp = np.tile(base, (n, 1))
        dp[1::3, 4:6] = DruckerPrager.new(3e5, 0.3).as_array()[4:6]
        state = np.tile(np.array([1.0, 1.0, 0.0], np.float32), (n, 1))
        state[2::3] = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.0, 2.0, n), rng.uniform(-0.2, 0.2, n)], 1)[2::3]
        ch, so, Fo = probes[dim].dp(dp, state, F32)
        F = T.mat(F32, dim)
        res = T.dp_outcomes64(dp.astype(np.float64), state.astype(np.float64), F, T.svd_lapack(F32))
        allowed = T.dp_allowed(res)
        amb = np.array([len(a) > 1 for a in allowed])
        iso = res["amb_zero"]            # isotropic strain (c I, c R, tied values): the all_zero test is a coin toss by design
        n_amb += int((amb & ~iso).sum())
        n_tot += int((~iso).sum())
        worst = (0.0, -1)
        for i in range(n):
            br, w = T.dp_match(res, i, ch[i], T.mat(Fo[i][None], dim)[0], so[i].astype(np.float64), np.linalg.norm(F[i]))
            if br is None or not w <= 1.0:
                fails.append(f"{fam} #{i}: changed={bool(ch[i])} matches none of {sorted(allowed[i])} within the bounds "
                             f"(best {br}: {w:.3g} x bound; fp64 branch {res['branch'][i]}, trace {res['tr'][i]:.3e}, "
                             f"gamma {res['gamma'][i]:.3e}; F = {F[i].tolist()}, state {state[i].tolist()})")
            elif w > worst[0]:
                worst = (w, i)
        report_margin(f"dp{dim}d {fam}: worst output error / bound (branch-matched)", worst[0], 1.0, ambiguous=int(amb.sum()), n=n)
        # the fp64 C oracle takes the fp64 branch with the same outputs (a second route to the same truth)
        for i in np.nonzero(~amb)[0][:64]:
            c, st_c, F_c = orc.drucker_prager_project(dp[i].astype(np.float64), state[i].astype(np.float64), F32[i].astype(np.float64))
            o = res["out"][res["branch"][i]]
            assert c == (res["branch"][i] != "N"), (fam, i)
            assert np.allclose(T.mat(F_c[None], dim)[0], o["F"][i], rtol=1e-9, atol=1e-9 * np.linalg.norm(F[i])), (fam, i)
            assert np.allclose(st_c, o["state"][i], rtol=1e-9, atol=1e-9), (fam, i)
    # isotropic strain is where the band is expected; anywhere else it must stay rare
    report_margin(f"dp{dim}d decision-ambiguous fraction outside isotropic strain", n_amb / n_tot, 0.05, count=n_amb)
    assert n_amb <= 0.05 * n_tot
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:20])
    # inverted F: NaN-ness only (out of scope: log of a negative singular value in the reference too)
    inv = np.concatenate([T.catalogue(dim, seed=2)[k] for k in ("inverted_distinct", "inverted_tied")])
    n = len(inv)
    ch, so, Fo = probes[dim].dp(np.tile(base, (n, 1)), np.tile(np.array([1.0, 1.0, 0.0], np.float32), (n, 1)), inv)
    for i in range(n):
        c, st_c, F_c = orc.drucker_prager_project(base.astype(np.float64), np.array([1.0, 1.0, 0.0]), inv[i].astype(np.float64))
        assert bool(np.isnan(Fo[i]).any()) == bool(np.isnan(F_c).any()), i


def _slow_matrices(dim, n, rng):
    """Matrices SELECTED BY EMULATION as ones that keep device_math.h's Jacobi sweeping for all five sweeps: an fp32 numpy
    restatement of its stopping rule, with IEEE division / sqrt and numpy's summation where the kernel uses the hardware's
    approximate rcp / sqrt / rsq and contracted sums (about 1 % of Gaussian matrices). That the device keeps its wave in
    the loop for them is not observed, only likely: the two rules differ by round-off."""
    out = []
    tries = 0
    while len(out) < n and tries < 50:
        tries += 1
        F = rng.normal(size=(4096, dim * dim)).astype(np.float32)
        sw = _emulated_sweeps(F, dim)
        out += list(F[sw >= 5])
    return np.array(out[:n], np.float32) if out else np.zeros((0, dim * dim), np.float32)


def _emulated_sweeps(F32, dim):
    a = T.mat(F32, dim).astype(np.float32).transpose(0, 2, 1).copy()   # a[n, col, row]
    n = len(a)
    live = np.ones(n, bool)
    sweeps = np.zeros(n, int)
    f = np.float32
    with np.errstate(all="ignore"):
        for sweep in range(5):
            sweeps[live] += 1
            rotated = np.zeros(n, bool)
            for p, q in ((0, 1), (0, 2), (1, 2)):
                al = (a[:, p] * a[:, p]).sum(1, dtype=f)
                be = (a[:, q] * a[:, q]).sum(1, dtype=f)
                ga = (a[:, p] * a[:, q]).sum(1, dtype=f)
                zeta = (be - al) / (f(2) * ga)
                t = np.copysign(f(1), zeta) / (np.abs(zeta) + np.sqrt(f(1) + zeta * zeta))
                skip = ~live | ~(np.abs(ga) > f(1e-30)) | ~(ga * ga > f(1e-15) * al * be) | np.isnan(t)
                c = f(1) / np.sqrt(f(1) + t * t)
                s = c * t
                ap, aq = a[:, p].copy(), a[:, q].copy()
                m = ~skip
                a[m, p] = c[m, None] * ap[m] - s[m, None] * aq[m]
                a[m, q] = s[m, None] * ap[m] + c[m, None] * aq[m]
                rotated |= m & (ga * ga > f(1e-13) * al * be)
            live &= rotated
    return sweeps + live.astype(int)     # 6 = still live after the fifth sweep


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [3, 2])
def test_svd_lane_independence(probes, hip_libs, dim):
    """device_math.h svd: 'a lane's result depends on its own matrix only' — what the launch-shape bit-identity tests
    rest on. Every catalogue matrix runs in lane 0 of a wave of 63 copies of itself and in lane 0 of a wave whose other 63
    lanes are matrices an emulation of the stopping rule selects as sweeping to the cap (_slow_matrices): the bits of U,
    S, V must be equal."""
    rng = np.random.default_rng(5 + dim)
    F32 = np.concatenate(list(_families(dim, False).values()))
    n = len(F32)
    # (2D: two fixed rotations, no sweep loop and no vote — the claim holds trivially and is checked all the same)
    slow = _slow_matrices(dim, 63, rng) if dim == 3 else T.catalogue(dim, seed=3)["ill_conditioned"]
    if dim == 3:
        report_margin("lane independence: slow neighbours found (emulated 5 sweeps)", 63 - len(slow), 63)
        assert len(slow) == 63
    slow = np.resize(slow, (63, dim * dim))
    same = np.repeat(F32[:, None, :], 64, 1).reshape(-1, dim * dim)
    mixed = np.concatenate([F32[:, None, :], np.broadcast_to(slow[None], (n, 63, dim * dim))], 1).reshape(-1, dim * dim)
    a = probes[dim].svd(same)
    b = probes[dim].svd(mixed)
    for x, y, name in zip(a, b, "USV"):
        x0 = x.reshape(n, 64, -1)
        y0 = y.reshape(n, 64, -1)[:, 0]
        assert np.array_equal(x0[:, 0].view(np.uint32), y0.view(np.uint32)), f"{name}: lane result depends on its neighbours"
        assert (x0.view(np.uint32) == x0[:, :1].view(np.uint32)).all(), f"{name}: copies of one matrix differ inside a wave"
