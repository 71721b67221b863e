"""CPU: the fp64 truth of the snow update (tests/snow_truth.py) has the properties of the rule, its judge passes an honest fp32
restatement (numpy, LAPACK's fp32 SVD: another algorithm than the kernel's, and no constant here has seen a HIP kernel) and catches
deliberate mistakes in it, the GPU scenes meet their conditions from the truth alone, and what surrounds the kernel — the Python
dataclass, the constants, the scene key, the header's prose — is in place."""
import functools

import numpy as np
import pytest

import abi
import devmath_truth as DM
import plastic_truth as PT
import snow_truth as ST
import transfer_truth as T
from wgsparkl_amd import MpmData, models, scenes
from wgsparkl_amd.sharded import NativeShard

DP = np.array([ST.THETA_C, ST.THETA_S, ST.XI, ST.CAP, 1.0, 0.0])
LO, HI = 1.0 - ST.THETA_C, 1.0 + ST.THETA_S


def _F(d, s, seed=0):
    return DM._usv(np.random.default_rng(seed), np.asarray(s, np.float64))


def _rows(n):
    return np.tile(DP, (n, 1))


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("d", [2, 3])
def test_inside_the_box_nothing_changes_and_the_update_is_the_elastic_one(d):
    rng = np.random.default_rng(d)
    n = 200
    F = _F(d, rng.uniform(LO + 1e-6, HI - 1e-6, (n, d)), 1)
    jp = rng.uniform(0.5, 1.5, n)
    FE, jp2, sh, (U, s, V) = ST.project64(F, _rows(n), jp)
    assert np.abs(FE - F).max() <= 64 * T.U64 and np.abs(jp2 - jp).max() <= 64 * T.U64
    lam, mu = np.full(n, 3.0e4), np.full(n, 2.0e4)
    hf, _ = ST.hardening64(_rows(n), np.ones(n))
    assert np.all(hf == 1.0)                                   # Jp = 1: the coefficients as they are
    tau = DM.tau_corotated64(FE, lam * hf, mu * hf, U, sh)
    assert np.abs(tau - DM.tau_corotated64(F, lam, mu, U, s)).max() <= 1e-9 * np.abs(tau).max()


@pytest.mark.parametrize("d", [2, 3])
def test_projection_is_idempotent_and_keeps_the_total_volume(d):
    rng = np.random.default_rng(10 + d)
    n = 300
    F = _F(d, np.exp(rng.uniform(np.log(0.3), np.log(3.0), (n, d))), 2)
    jp = rng.uniform(0.3, 1.5, n)
    FE, jp2, sh, _ = ST.project64(F, _rows(n), jp)
    assert np.all((sh >= LO) & (sh <= HI))
    # det(F_trial) Jp = det(F_E) Jp' for s > 0
    assert np.abs(np.linalg.det(F) * jp - np.linalg.det(FE) * jp2).max() <= 1e-12 * np.abs(np.linalg.det(F) * jp).max()
    FE2, jp3, sh2, _ = ST.project64(FE, _rows(n), jp2)
    assert np.abs(FE2 - FE).max() <= 256 * T.U64 and np.abs(jp3 - jp2).max() <= 256 * T.U64 * jp2.max()


def test_hardening_is_monotone_in_jp_and_saturates():
    jp = np.linspace(-0.5, 2.5, 601)
    hf, e = ST.hardening64(_rows(len(jp)), jp)
    assert np.all(np.diff(hf) <= 0.0) and np.all(hf <= np.exp(ST.CAP))
    assert np.all(hf[jp <= 1.0 - ST.CAP / ST.XI] == np.exp(ST.CAP))          # the cap: xi (1 - Jp) >= h3
    assert hf[np.argmin(np.abs(jp - 1.0))] == pytest.approx(1.0, abs=1e-12)
    assert set(np.round(ST.XI * (1.0 - np.asarray(ST.JP_IN)), 6)) >= {0.0, 4.0, -4.0, 7.0, 10.0}    # the GPU scenes' Jp_in: below, at and beyond the cap


@pytest.mark.parametrize("d", [2, 3])
def test_a_vanished_singular_value_gives_zero_and_an_inverted_matrix_a_positive_volume(d):
    s = np.full((4, d), 1.1)
    s[0, -1] = 0.0
    s[1, -1] = -0.7
    s[2, -1] = -1.1        # tied with the others in magnitude
    s[3, -1] = 1e-9
    rng = np.random.default_rng(3)
    U, V = DM.rotations(rng, 4, d), DM.rotations(rng, 4, d)
    F = (U * s[:, None, :]) @ np.transpose(V, (0, 2, 1))
    FE, jp2, sh, _ = ST.project64(F, _rows(4), np.full(4, 0.8), svd=(U, s, V))      # (the SVD as drawn: s = 0 exactly)
    assert jp2[0] == 0.0 and np.all(jp2 >= 0.0) and jp2[1] > 0.0
    assert np.all(np.linalg.det(FE) > 0.0) and np.all(sh.min(1) == LO)        # back to the lower edge of the box
    sn = ST.Snow(F, _rows(4).astype(np.float32), np.tile([0.8, 1.0, 0.0], (4, 1)), np.zeros((4, 2)))
    assert list(sn.ambiguous) == [True, False, True, True]                   # the direction of a vanished or sign-tied value is arbitrary


# ------------------------------------------------------------------------------------------------ an fp32 restatement and its mistakes
class Run:
    def __init__(self, case, d):
        self.sc, self.fam = ST.scene(case, d)
        self.ps = ps = self.sc["particles"]
        self.d = d
        self.inp = T.Inputs.of(ps)
        prm = self.sc["params"]
        self.pt = T.substep(self.inp, self.sc["cell_width"], prm.dt, prm.gravity)[2]
        self.F_trial32 = T.unmat(self.pt.F).astype(np.float32)                # stands for the kernel's own trial matrix
        self.sn = ST.Snow(T.mat(self.F_trial32, d), ps.dp, ps.dp_state, ps.phase)


@functools.lru_cache(maxsize=None)
def _run(case, d):
    return Run(case, d)


def _restate(r: Run, mistake=None):
    """the update in fp32 numpy from the trial state of the truth (x, v, grad in fp64 rounded once): sgesdd, the sign on the smallest
    value, clamp, Jp', recomposition, hardening and stress, every product rounded to fp32"""
    f32 = np.float32
    ps, d, n = r.ps, r.d, r.ps.n
    F = T.mat(r.F_trial32, d).astype(f32)
    U, s, Vt = np.linalg.svd(F)
    V = np.transpose(Vt, (0, 2, 1)).copy()
    fu, fv = np.linalg.det(U.astype(np.float64)) < 0, np.linalg.det(V.astype(np.float64)) < 0
    U[fu, :, -1] *= f32(-1)
    V[fv, :, -1] *= f32(-1)
    s = s.copy()
    s[fu != fv, -1] *= f32(-1)
    phase = ps.phase[:, 0].copy()
    breakable = (phase > 0) & (ps.phase[:, 1] > 0)
    phase[breakable & (np.abs(s).max(1) > ps.phase[:, 1])] = 0.0
    cand = (phase == 0) & (ps.dp[:, 4] != 0)
    lo, hi = (f32(1) - ps.dp[:, 0])[:, None], (f32(1) + ps.dp[:, 1])[:, None]
    sh = np.clip(np.abs(s) if mistake == "unsigned clamp" else s, lo, hi).astype(f32)
    if mistake == "unsigned clamp":
        sh = (np.where(s < 0, f32(-1), f32(1)) * sh).astype(f32)
    jp_in = ps.dp_state[:, 0]
    jp = (jp_in * np.prod(np.abs(s), 1, dtype=f32) / np.prod(sh, 1, dtype=f32)).astype(f32)
    FE = ((U * sh[:, None, :]) @ np.transpose(V, (0, 2, 1))).astype(f32)
    hf = np.exp(np.minimum(ps.dp[:, 2] * (f32(1) - (jp_in if mistake == "old Jp in hf" else jp)), ps.dp[:, 3])).astype(f32)
    hf = np.where(cand, hf, f32(1))
    Fo = np.where(cand[:, None, None], FE, F)
    so = np.where(cand[:, None], sh, s)
    lam = (ps.lambda_ * (f32(1) if mistake == "hf on mu only" else hf)).astype(f32)
    mu = (ps.mu * hf).astype(f32)
    tau = DM.tau_corotated64(Fo.astype(np.float64), lam.astype(np.float64), mu.astype(np.float64), U.astype(np.float64), so.astype(np.float64))
    coeff = r.inp.vol * r.pt.invd * r.pt.dt
    Cn = r.pt.grad * r.inp.m[:, None, None] - tau * coeff[:, None, None]
    st = ps.dp_state.copy()
    st[cand, 0] = jp[cand]
    if mistake == "state word 1 touched":
        st[cand, 1] += f32(0.5)
    ph = ps.phase.copy()
    ph[:, 0] = phase
    return dict(pos=r.pt.x.astype(f32), vel=r.pt.vel.astype(f32), def_grad=T.unmat(Fo.astype(np.float64)).astype(f32),
                affine=T.unmat(Cn).astype(f32), dp_state=st, phase=ph)


def _verdict(r: Run, got):
    fails = []
    jd = ST.judge("restated", r.sn, got, fails, F_trial32=r.F_trial32)
    ST.check_particles("restated", r.pt, got, jd, fails)
    ST.report_ambiguous("restated", jd, r.sn, fails)
    return fails, jd


@pytest.mark.parametrize("case,d", [("layout1_switch_per_particle", 2), ("layout0_parameters_per_particle", 3), ("layout1_fracture", 3)])
def test_an_honest_fp32_restatement_fits_every_bound(case, d):
    r = _run(case, d)
    fails, jd = _verdict(r, _restate(r))
    assert not fails, "\n".join(fails)
    assert jd.cand.sum() > 0.4 * r.ps.n and ((~jd.cand).sum() > 0.1 * r.ps.n or case.startswith("layout0"))


@pytest.mark.parametrize("mistake,said", [("old Jp in hf", "C' of the snow particles"), ("unsigned clamp", "snow"), ("hf on mu only", "C' of the snow particles"),
                                          ("state word 1 touched", "state word 1 or 2")])
def test_deliberate_mistakes_are_caught(mistake, said):
    r = _run("layout1_switch_per_particle", 3)
    fails, _ = _verdict(r, _restate(r, mistake))
    assert any(said in f for f in fails), (mistake, fails[:3])


# ------------------------------------------------------------------------------------------------ the scenes
@pytest.mark.parametrize("case,d", ST.CASE_IDS)
def test_the_gpu_scenes_meet_their_conditions_from_the_truth_alone(case, d):
    """the share of particles judged without their direction, or inside the fracture band, is under plastic_truth.AMBIGUOUS_MAX; every
    axis meets singular values below, inside and above the box, inverted and cut-off ones included; every Jp_in occurs"""
    sc, fam = ST.scene(case, d)
    ps = sc["particles"]
    inp = T.Inputs.of(ps)
    pt = T.substep(inp, sc["cell_width"], sc["params"].dt, sc["params"].gravity)[2]
    sn = ST.Snow(T.mat(T.unmat(pt.F).astype(np.float32), d), ps.dp, ps.dp_state, ps.phase)
    cand = sn.cand64 | (sn.fr.amb_frac & sn.has)
    amb = (cand & sn.ambiguous) | sn.fr.amb_frac
    assert amb.sum() <= PT.AMBIGUOUS_MAX * ps.n, (case, d, int(amb.sum()), ps.n)
    assert (cand & sn.ambiguous).sum() >= 3, "no hazardous matrix left in the scene"
    s = sn.svd[1][sn.cand64]
    lo, hi = ST.box(sn.dp[sn.cand64])
    for k in range(d):
        assert min((s[:, k] < lo).sum(), ((s[:, k] >= lo) & (s[:, k] <= hi)).sum(), (s[:, k] > hi).sum()) >= 10, (case, d, k)
    assert (s.min(1) < 0).sum() >= 10 and (np.abs(s).min(1) <= DM.CUTOFF * np.abs(s).max(1)).sum() >= 2
    assert {float(x) for x in np.unique(ps.dp_state[:, 0])} == {float(np.float32(x)) for x in ST.JP_IN}
    assert pt.near_cap.sum() <= PT.NEAR_MAX * ps.n
    if ST.CASES[case][1]:
        assert 0 < sn.fr.broken.sum() < sn.fr.breakable.sum()
    if ST.CASES[case][0] == 1:
        assert 0.2 * ps.n < (~sn.has).sum() < 0.5 * ps.n


def test_the_fracture_rule_is_one_truth_inside_snow_and_inside_drucker_prager():
    """plastic_truth.Fracture built by Snow and by Plastic from the same (F, phase) agrees array for array, on a snow scene and on a
    Drucker-Prager scene; Snow computes no Drucker-Prager outcome."""
    for mod, case in ((ST, "layout1_fracture"), (PT, "mode1_fracture_corotated")):
        sc, _ = mod.scene(case, 3)
        ps = sc["particles"]
        pt = T.substep(T.Inputs.of(ps), sc["cell_width"], sc["params"].dt, sc["params"].gravity)[2]
        F = T.mat(T.unmat(pt.F).astype(np.float32), 3)
        sn = ST.Snow(F, _rows(ps.n), ps.dp_state, ps.phase)
        pl = PT.Plastic(F, None, ps.dp, ps.dp_state, ps.phase)
        assert isinstance(sn.fr, PT.Fracture) and isinstance(pl.fr, PT.Fracture) and not isinstance(sn.fr, PT.Plastic)
        assert 0 < sn.fr.broken.sum() < sn.fr.breakable.sum()
        for k in ("s_max", "phase_in", "max_stretch", "breakable", "broken", "amb_frac", "phase64", "f_err"):
            assert np.array_equal(getattr(sn.fr, k), getattr(pl.fr, k)) and getattr(pl, k) is getattr(pl.fr, k), k
        assert all(np.array_equal(a, b) for a, b in zip(sn.fr.svd, pl.fr.svd)) and sn.svd[1] is sn.fr.svd[1]
        assert not any(hasattr(o, k) for o in (sn, sn.fr) for k in ("res", "allowed")) and hasattr(pl, "res")


# ------------------------------------------------------------------------------------------------ around the kernel
def test_snow_dataclass_packs_the_six_slots_and_checks_the_preconditions():
    s = models.Snow()
    assert s.as_array().dtype == np.float32 and list(s.as_array()) == [np.float32(2.5e-2), np.float32(7.5e-3), 10.0, 5.0, 1.0, 0.0]
    assert (s.h0, s.h1, s.h2, s.h3, s.lambda_, s.mu) == (2.5e-2, 7.5e-3, 10.0, 5.0, 1.0, 0.0)
    for bad in (dict(theta_c=-0.1), dict(theta_c=1.0), dict(theta_c=float("nan")), dict(theta_s=-1e-3), dict(theta_s=float("inf")),
                dict(xi=float("inf")), dict(max_exponent=float("nan")), dict(theta_c=1.0 - 1e-9)):
        with pytest.raises(ValueError):
            models.Snow(**bad)
    models.Snow(theta_c=0.0, theta_s=0.0, xi=-3.0, max_exponent=-1.0)      # the edges are allowed
    ps = scenes.snowball(dim=2)["particles"]
    assert np.array_equal(ps.dp[0], s.as_array()) and ps.has_plasticity.all()


def test_the_header_states_the_snow_rule_its_declarations_and_its_two_values():
    """What only snow can know of include/wgsparkl_hip.h (that its constants, prototypes and mirrors agree is tests/test_abi.py's, for
    every entry of the header): the prose the section promises, its three declaration lines verbatim, and the two values."""
    raw = abi.read(abi.HEADER_PATH)
    assert "wgs_status wgs_set_plasticity_model(wgs_data *data, int32_t kind);" in raw
    assert "wgs_status wgs_get_plasticity_model(wgs_data *data, int32_t *out);" in raw
    assert "enum { WGS_PLASTICITY_DRUCKER_PRAGER = 0, WGS_PLASTICITY_SNOW = 1 };" in raw
    text = " ".join(raw.replace("\n *", " ").split())
    section = text[text.index("/* Snow plasticity."):text.index("enum { WGS_PLASTICITY_DRUCKER_PRAGER")]
    for phrase in ("0 <= theta_c < 1, theta_s >= 0, xi and h3 finite", "hf is taken of the UPDATED Jp"):
        assert phrase in section, phrase
    assert (models.PLASTICITY_DRUCKER_PRAGER, models.PLASTICITY_SNOW) == (0, 1)


def test_library_exports_the_switch(hip_libs):
    for dim in (2, 3):
        lib, _ = hip_libs.load(dim)
        assert lib.wgs_set_plasticity_model(None, 0) == hip_libs.ERR_INVALID_ARGUMENT
        assert lib.wgs_get_plasticity_model(None, None) == hip_libs.ERR_INVALID_ARGUMENT


def test_from_scene_applies_the_plasticity_key_behind_the_model_and_a_slab_refuses_it(monkeypatch):
    log = []

    class Recorder:
        def __getattr__(self, name):
            if not name.startswith("set_"):
                raise AttributeError(name)
            return lambda value: log.append((name, value))

    monkeypatch.setattr(MpmData, "new", classmethod(lambda cls, *a: log.append(("new", a[-1])) or Recorder()))
    sc = dict(params="p", particles="ps", colliders=[], cell_width=0.5, grid_capacity=64, model=0, plasticity=1, fluid_gamma=5.0, walls="w")
    MpmData.from_scene("pipe", sc)
    assert log == [("new", 0), ("set_plasticity_model", 1), ("set_fluid_eos", 5.0), ("set_domain_walls", "w")]
    del log[:]
    MpmData.from_scene("pipe", sc, plasticity=None)
    assert [c[0] for c in log] == ["new", "set_fluid_eos", "set_domain_walls"]
    with pytest.raises(ValueError, match="plasticity"):
        NativeShard.from_scene("pipe", dict(sc, walls=None, global_ids="ids", partition=None), 0)
    sb = scenes.snowball(dim=3)
    assert sb["plasticity"] == models.PLASTICITY_SNOW and sb["walls"][0].type == models.WALL_STICKY and sb["colliders"] == []
