"""-m gpu: snow — the singular-value clamp with hardening (wgs_set_plasticity_model(WGS_PLASTICITY_SNOW); the MODEL 4 instantiations of
the fused G2P, g2p_body.inc) — per particle against the fp64 truth of tests/snow_truth.py (validated on the CPU by
tests/test_snow_truth.py), and what follows the rule through the layers: read-outs, restart, statuses, a scene.

The per-particle check is plastic_truth's isolated one: the same state stripped of plasticity runs beside the snow run; P2G does not
read the plastic state, so the twin's x and v are the snow run's bit for bit and its def_grad is the kernel's own fp32 F_trial. Every
particle that did not pass the gate holds exactly that matrix; the truth of the others is taken of that exact matrix."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest

import devmath_truth as DM
import diag_truth as dt
import plastic_truth as PT
import snow_truth as ST
import transfer_truth as T
from gpu_common import _start, _step, checked_plastic_substep, plastic_twin, steady_plastic_substep
from helpers import PLASTIC_FIELDS, _digest, assert_same_bits, debug, new_data, report_margin
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd.models import MODEL_COROTATED, MODEL_FLUID, MODEL_NEO_HOOKEAN, PLASTICITY_DRUCKER_PRAGER, PLASTICITY_SNOW, Snow
from wgsparkl_amd.sharded import lockstep_slabs

pytestmark = pytest.mark.gpu

def _check(tag, sc, before, got, twin, grid, poses, fam, fails):
    """one substep from `before` (a ParticleSet with its dp_state and phase) to `got`, `twin` the stripped run's result: gpu_common's
    checks of every plastic substep, then the snow verdict on the kernel's own F_trial"""
    _, iso, keep = checked_plastic_substep(tag, sc, before, got, twin, grid, poses, 0, fails)
    sn = ST.Snow(T.mat(twin.def_grad, before.dim), before.dp, before.dp_state, before.phase)
    jd = ST.judge(f"{tag} isolated", sn, got, fails, F_trial32=twin.def_grad)
    ST.report_ambiguous(f"{tag} isolated", jd, sn, fails)
    ST.check_particles(f"{tag} isolated G2P", iso, got, jd, fails, sel=keep)
    report_margin(f"{tag}: particles through the projection (required / found)", int(0.3 * before.n), int(jd.cand.sum()))
    assert jd.cand.sum() >= 0.3 * before.n
    return sn, jd


@pytest.mark.parametrize("case,d", ST.CASE_IDS)
def test_one_substep_of_snow_per_particle(hip_libs, monkeypatch, case, d):
    dbg = ST.CASES[case][3]
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    with debug(monkeypatch, dbg) if dbg is not None else contextlib.nullcontext():
        sc, fam = ST.scene(case, d)
        ps = sc["particles"]
        pipe, data = _start(sc)
        assert data.plasticity_model() == PLASTICITY_SNOW
        poses = data.read_body_poses()
        got = _step(pipe, data)
        grid = data.read_grid()
        twin = plastic_twin(sc)
    fails = []
    sn, jd = _check(f"{case} {d}D", sc, ps, got, twin, grid, poses, fam, fails)
    assert not fails, "\n".join(fails)
    if ST.CASES[case][0] == 1:                  # the switch is per particle: those with it off are elastic corotated particles
        off = ps.dp[:, 4] == 0
        assert off.sum() > 0.2 * ps.n and not jd.cand[off].any()
    if ST.CASES[case][1]:
        broke = (got.phase[:, 0] == 0) & (ps.phase[:, 0] != 0)
        report_margin(f"{case} {d}D: particles broken and projected in the checked substep (required / found)", 10, int((broke & jd.cand).sum()))
        assert (broke & jd.cand).sum() >= 10


@pytest.mark.parametrize("case,d,h", ST.STEADY)
def test_the_sixteenth_substep_after_fifteen(hip_libs, case, d, h):
    sc, fam = ST.scene(case, d, h=h, steady=True)
    before, got, twin, grid, _, _ = steady_plastic_substep(sc, 15)
    fails = []
    sn, jd = _check(f"steady state {case} {d}D", sc, before, got, twin, grid, None, fam, fails)
    assert not fails, "\n".join(fails)
    again = jd.cand & (before.dp_state[:, 0] != sc["particles"].dp_state[:, 0])
    report_margin(f"steady state {case} {d}D: clamped in the checked substep and before it (required / found)", 20, int((again & sn.clamped).sum()))
    assert (again & sn.clamped).sum() >= 20


# ------------------------------------------------------------------------------------------------ same bits
@pytest.mark.parametrize("d", [2, 3])
def test_reruns_launch_shapes_and_a_restart_give_the_same_bits(hip_libs, monkeypatch, d):
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    sc, _ = ST.scene("layout2", d, steady=True, h=0.5)

    def run(k=8):
        pipe, data = _start(sc)
        pipe.step(data, 3)
        data.sync()
        pipe.step(data, k - 3)
        data.sync()
        return data

    a = run()
    want = _digest(a)
    assert _digest(run()) == want
    for switch in ("NO_UNIFORM", "G2P_TWO_PASSES", "REBIN_LAUNCH", "GU_OWN_LAUNCH"):
        with debug(monkeypatch, switch):
            assert _digest(run()) == want, switch
    # a restart: read-back + plastic state -> new data + set_plastic_state + the switch continues bit for bit
    b = run(5)
    snap = b.read_particles()
    pipe, c = new_data(sc, particles=snap)
    c.set_plastic_state(snap.dp_state)
    assert c.plasticity_model() == PLASTICITY_SNOW
    for x in (b, c):
        pipe.step(x, 3)
        x.sync()
    assert_same_bits(b.read_particles(), c.read_particles(), PLASTIC_FIELDS + ("phase",))
    assert _digest(b) == _digest(c) == want


def test_the_two_register_budgets_of_the_pair_give_the_same_bits(hip_libs, monkeypatch):
    """test_gpu_bit_identity's sand between a floor and four walls, as snow: after the first wgs_sync the fused G2P runs the pair
    compiled for 2 waves per SIMD; NO_G2P_DENSE keeps the 3-waves one, G2P_TWO_LAUNCHES the two bodies as launches of their own."""
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    sc = scenes.sand_column(nx=40, ny=60, nz=40, with_walls=True)
    sc["particles"].pos[:, 1] -= 5.8
    sc["particles"].dp[:] = Snow().as_array()
    sc["particles"].def_grad[:] *= np.float32(1.05)        # beyond the box on every axis: the first substep clamps every particle
    sc["plasticity"] = PLASTICITY_SNOW

    def run():
        pipe, data = new_data(sc)
        pipe.step(data, 4)
        data.sync()
        st = data.stats()
        assert st["num_near_collider_blocks"] * 2 >= st["num_active_blocks"]     # the switch condition of host_substep.inc plan_g2p
        pipe.step(data, 8)
        data.sync()
        return data.read_particles()

    a = run()
    assert np.isfinite(a.pos).all() and (a.dp_state[:, 0] != 1.0).sum() > 1000
    for switch in ("NO_G2P_DENSE", "G2P_TWO_LAUNCHES"):
        with debug(monkeypatch, switch):
            assert_same_bits(a, run(), PLASTIC_FIELDS, switch)


# ------------------------------------------------------------------------------------------------ read-outs
@pytest.mark.parametrize("case,d", [("layout1_switch_per_particle", 3), ("layout2", 2), ("layout0_parameters_per_particle", 3)])
def test_field_readout_and_elastic_sum_take_the_hardened_coefficients(hip_libs, case, d):
    sc, _ = ST.scene(case, d)
    pipe, data = _start(sc)
    got = _step(pipe, data, 2)
    n = got.n
    snow = (got.phase[:, 0] == 0) & (got.dp[:, 4] != 0)
    hf, e = ST.hardening64(got.dp, got.dp_state[:, 0])
    hf = np.where(snow, hf, 1.0)
    rel = np.where(snow, DM.C_DP * T.U32 * (np.abs(got.dp[:, 2].astype(np.float64) * got.dp_state[:, 0]) + np.abs(e) + 1.0), 0.0)
    F = T.mat(got.def_grad.astype(np.float64), d)
    lam, mu = got.lambda_.astype(np.float64) * hf, got.mu.astype(np.float64) * hf
    fl = data.particle_fields()
    assert np.all(fl.model == MODEL_COROTATED)
    svd64 = DM.svd_lapack(got.def_grad)
    # (a hardened coefficient is an fp32 number: below FLT_MIN 2^24 it has lost its relative precision, or is flushed to zero. Jp' of
    # the catalogue's large matrices is 1e9 and hf = exp(-1e10): those particles are held to a stress of that size, the others to C_TAU)
    tiny = 2.0 ** -102
    lost = (np.minimum(lam, mu) < tiny) & snow
    fails = DM.check_tau(f"fields {case} {d}D", 0, fl.stress[~lost].astype(np.float64), F[~lost], lam[~lost], mu[~lost], tuple(a[~lost] for a in svd64))
    assert not fails, "\n".join(fails)
    floor = np.full(int(lost.sum()), tiny)
    assert np.all(np.linalg.norm(fl.stress[lost], axis=(1, 2)) <= 2.0 * DM.tau_scales(0, F[lost], floor, floor, svd64[1][lost])) and lost.sum() < 0.1 * n
    # the stress is NOT that of the stored coefficients where hf says so
    t_plain = DM.tau_corotated64(F, got.lambda_.astype(np.float64), got.mu.astype(np.float64), svd64[0], svd64[1])
    far = snow & (np.abs(hf - 1.0) > 0.1) & DM.tau_unique(svd64[1])
    off = np.linalg.norm(fl.stress - t_plain, axis=(1, 2)) > 4.0 * DM.C_TAU * T.U32 * DM.tau_scales(0, F, lam, mu, svd64[1])
    assert far.sum() > 0.2 * n and off[far].mean() > 0.5
    # WGS_SUM_ELASTIC: the diagnostics' own bound (test_gpu_diagnostics: rounding of the fixed-point sum + 2 x 256 roundings of the fp64
    # evaluation) + what the kernel's fp32 hf may differ from the fp64 one of the stored Jp, relative `rel` of each snow particle's term
    dg = data.diagnostics(_ffi.DIAG_PARTICLES | _ffi.DIAG_ENERGY)
    hard = got.copy()
    hard.lambda_, hard.mu = lam.astype(np.float64), mu.astype(np.float64)
    t, mag = dt.terms(hard, sc["cell_width"], sc["params"].gravity, MODEL_COROTATED, True)
    keep = dt.finite_mask(hard)
    s = dg.sums["elastic"]
    truth = math.fsum(t["elastic"][:, 0])
    bound = n * 2.0 ** (s.exponent - 1) + 2 * 256 * T.U64 * math.fsum(mag["elastic"][:, 0]) + math.fsum(mag["elastic"][:, 0] * rel[keep])
    err = abs(float(s.value[0]) - truth)
    report_margin(f"elastic sum {case} {d}D |value - truth|", err, bound)
    assert err <= bound
    plain = math.fsum(dt.terms(got, sc["cell_width"], sc["params"].gravity, MODEL_COROTATED, True)[0]["elastic"][:, 0])
    # (layout 1: the particles with the switch off keep the catalogue's wild F and carry the sum; the snow particles' F_E is in the box)
    assert abs(plain - truth) > 100.0 * bound or case.startswith("layout1"), "the scene does not tell hardened from stored coefficients"
    # the other sums and the digest do not know the switch; elastic particles read out bit for bit as without it
    raw = fl.raw.copy()
    data.set_plasticity_model(PLASTICITY_DRUCKER_PRAGER)
    dg0 = data.diagnostics(_ffi.DIAG_ALL)
    fl0 = data.particle_fields()
    data.set_plasticity_model(PLASTICITY_SNOW)
    dg1 = data.diagnostics(_ffi.DIAG_ALL)
    assert np.array_equal(raw[~snow], fl0.raw[~snow]) and not np.array_equal(raw[far], fl0.raw[far])
    assert dg0.digest == dg1.digest and dg1.sums["elastic"].value[0] == s.value[0]
    assert dg0.sums["elastic"].value[0] != s.value[0] or case.startswith("layout1")      # (layout 1: the sum is the other particles', above)
    for name in ("mass", "momentum", "kinetic", "kinetic_affine", "gravity_potential"):
        assert np.array_equal(dg0.sums[name].value, dg1.sums[name].value), name
    if case.startswith("layout1"):
        assert (~snow).sum() > 0.2 * n


# ------------------------------------------------------------------------------------------------ nothing else changes
@pytest.mark.parametrize("d", [2, 3])
def test_drucker_prager_data_does_not_notice_the_call(hip_libs, d):
    sc, _ = PT.scene("mode1_fracture_corotated", d)

    def run(call):
        pipe, data = _start(sc)
        if call:
            data.set_plasticity_model(PLASTICITY_DRUCKER_PRAGER)
        pipe.step(data, 8)
        data.sync()
        return _digest(data), data.particle_fields().raw

    (da, fa), (db, fb) = run(False), run(True)
    assert da == db and np.array_equal(fa, fb)
    # ... nor elastic data the snow rule: its step carries no plastic state
    el = PT.strip(sc)
    pipe, a = new_data(el)
    pipe, b = new_data(el, plasticity=PLASTICITY_SNOW)
    for x in (a, b):
        pipe.step(x, 8)
        x.sync()
    assert b.plasticity_model() == PLASTICITY_SNOW and _digest(a) == _digest(b)
    assert np.array_equal(a.particle_fields().raw, b.particle_fields().raw)
    assert a.diagnostics(_ffi.DIAG_ALL).sums["elastic"].value[0] == b.diagnostics(_ffi.DIAG_ALL).sums["elastic"].value[0]


@pytest.mark.parametrize("d", [2, 3])
def test_statuses(hip_libs, d):
    sc, _ = ST.scene("layout2", d, n=600)
    pipe, data = _start(sc, plasticity=None)
    lib, h = data.lib, data._h
    ok, invalid, unsupported = _ffi.WGS_OK, _ffi.ERR_INVALID_ARGUMENT, _ffi.ERR_UNSUPPORTED
    kind = C.c_int32(77)
    assert lib.wgs_get_plasticity_model(h, C.byref(kind)) == ok and kind.value == PLASTICITY_DRUCKER_PRAGER        # the default
    for bad in (2, -1, 1 << 20):
        assert lib.wgs_set_plasticity_model(h, bad) == invalid and lib.wgs_last_error()
    assert lib.wgs_set_plasticity_model(None, 0) == invalid and lib.wgs_get_plasticity_model(None, C.byref(kind)) == invalid
    assert lib.wgs_get_plasticity_model(h, None) == invalid and data.plasticity_model() == PLASTICITY_DRUCKER_PRAGER
    # snow is defined on the corotated stress
    data.set_constitutive_model(MODEL_NEO_HOOKEAN)
    assert lib.wgs_set_plasticity_model(h, PLASTICITY_SNOW) == unsupported and data.plasticity_model() == PLASTICITY_DRUCKER_PRAGER
    data.set_constitutive_model(MODEL_COROTATED)
    assert lib.wgs_set_plasticity_model(h, PLASTICITY_SNOW) == ok and data.plasticity_model() == PLASTICITY_SNOW
    for other in (MODEL_NEO_HOOKEAN, MODEL_FLUID):
        assert lib.wgs_set_constitutive_model(h, other) == unsupported and b"WGS_PLASTICITY_SNOW" in lib.wgs_last_error()
    assert lib.wgs_set_constitutive_model(h, MODEL_COROTATED) == ok and data.diagnostics(_ffi.DIAG_PARTICLES).model == MODEL_COROTATED
    assert lib.wgs_set_plasticity_model(h, PLASTICITY_DRUCKER_PRAGER) == ok and lib.wgs_set_constitutive_model(h, MODEL_NEO_HOOKEAN) == ok
    # a lockstep slab: WGS_ERR_UNSUPPORTED, in the words of the other single-domain calls; nothing changes
    shards, _ = lockstep_slabs(pipe, PT.strip(sc), 2, plasticity=None)
    for s in shards:
        assert lib.wgs_set_plasticity_model(s._h, PLASTICITY_SNOW) == unsupported and b"single-domain data only" in lib.wgs_last_error()
        assert lib.wgs_set_plasticity_model(s._h, PLASTICITY_DRUCKER_PRAGER) == unsupported
        assert lib.wgs_get_plasticity_model(s._h, C.byref(kind)) == ok and kind.value == PLASTICITY_DRUCKER_PRAGER
        s.close()


@pytest.mark.parametrize("d", [2, 3])
def test_a_snowball_hits_the_wall(hip_libs, d):
    sc = scenes.snowball(dim=d)
    pipe, data = new_data(sc)
    pipe.step(data, 50)
    data.sync()
    dg = data.diagnostics(_ffi.DIAG_ALL)
    got = data.read_particles()
    assert dg.num_nonfinite == 0 and data.stats()["overflow"] == 0
    jp = got.dp_state[:, 0]
    assert np.all(np.isfinite(jp)) and jp.min() > 0.0 and np.isfinite(jp.max())
    assert (np.abs(jp - 1.0) > 1e-3).sum() > 0.01 * got.n, "nothing was clamped: the ball did not reach the wall"
    plane = sc["walls"][0].plane * sc["cell_width"]
    assert got.pos[:, 0].min() >= plane - 1.5 * sc["cell_width"] and got.pos[:, 0].min() < plane + 2.0 * sc["cell_width"]
    assert np.array_equal(got.dp_state[:, 1:], sc["particles"].dp_state[:, 1:])
