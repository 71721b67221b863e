"""CPU: the fp64 truth of the plastic update in motion (tests/plastic_truth.py) and its bounds are right.

- the truth agrees per particle with the C fp64 oracle: the same decisions, F', dp_state and C' within C u64 of the stated scales;
- the C fp32 oracle, an honest fp32 implementation with another summation order and an fp64 SVD, lands inside every bound and
  every allowed-branch set, end to end (f_err = b_F) and isolated (the truth of its own elastic twin's F_trial, f_err = 0): the
  bounds are not too tight, and no constant here has seen a HIP kernel;
- the widening by f_err is a bound: random dF at |dF| = f_err move no branch's outputs, and no decision quantity, by more
  than devmath_truth.dp_outcomes64 states;
- deliberate mistakes in a numpy restatement of the update break a bound or a decision: the bounds are not vacuous;
- the scenes meet the conditions they are built for, from the truth alone."""
import functools

import numpy as np
import pytest

import cpic_truth as CP
import devmath_truth as DM
import plastic_truth as PT
import transfer_truth as T
from helpers import report_margin, run_oracle
from oracle import np_oracle

CASE_IDS = [(case, d) for case in sorted(PT.CASES) for d in (2, 3)]


class Run:
    """one scene through both C oracles (and the fp32 one's elastic twin), with the truths of each"""

    def __init__(self, case, d):
        self.case, self.d = case, d
        self.sc, self.fam = sc, _ = PT.scene(case, d)
        self.ps = ps = sc["particles"]
        self.model = sc["model"]
        self.inp = inp = T.Inputs.of(ps)
        h, prm = sc["cell_width"], sc["params"]
        if sc["colliders"]:
            mo = CP.Motion.of(sc["colliders"], d)
            o32, o64, tw = (CP.oracle_substep(s, t) for s, t in ((sc, np.float32), (sc, np.float64), (PT.strip(sc), np.float32)))
            self.arr32, self.arr64, self.twin32 = o32.arr, o64.arr, tw.arr
            self.pt = CP.substep(inp, h, prm.dt, prm.gravity, o32.fields, mo).particles
            self.pt64 = CP.substep(inp, h, prm.dt, prm.gravity, o64.fields, mo, u=T.U64).particles
            self.pt_iso = CP.substep(inp, h, prm.dt, prm.gravity, o32.fields, mo, own_grid=(o32.cells, o32.vm[:, :d])).particles
            self.skip = CP.Contact(inp, h, o32.fields, mo, T.U32).near_pen
            self.felt = int((o32.fields.paff != 0).sum())
        else:
            st32, st64, tw = run_oracle(sc, 1, np.float32), run_oracle(sc, 1, np.float64), run_oracle(PT.strip(sc), 1, np.float32)
            self.arr32, self.arr64, self.twin32 = st32.arr, st64.arr, tw.arr
            st, _, self.pt = T.substep(inp, h, prm.dt, prm.gravity)
            self.pt64 = T.substep(inp, h, prm.dt, prm.gravity, u=T.U64)[2]
            cells, mv = st32.grid_records()[:2]
            self.pt_iso = T.isolated(inp, st, cells, np.asarray(mv, np.float64)[:, :d], prm.dt)
            self.skip = np.zeros(ps.n, bool)
        self.pl = PT.Plastic(self.pt.F, self.pt.b_F, ps.dp, ps.dp_state, ps.phase)
        self.pl_in = PT.Plastic(inp.F, None, ps.dp, ps.dp_state, ps.phase)


@functools.lru_cache(maxsize=None)
def _run(case, d):
    return Run(case, d)


def _verdict(tag, pl, pt, got, model, skip=None, **kw):
    """(failures, Judged) of a result: the plastic verdict, and x, v, C' of every particle and F of the unprojected ones"""
    fails = []
    jd = PT.judge(tag, pl, got, fails, **kw)
    T.check_particles(tag, pt, got, model, fails, sel=None if skip is None or not skip.any() else ~skip, own_F=jd.changed)
    return fails, jd


@pytest.mark.parametrize("case,d", CASE_IDS)
def test_truth_matches_the_fp64_oracle_and_the_fp32_oracle_fits_the_bounds(oracle_libs, case, d):
    r = _run(case, d)
    tag = f"{case} {d}D"
    ps = r.ps
    # fp64: the same decisions, everything within C u64 of the scales
    pl64 = PT.Plastic(r.pt64.F, None, ps.dp, ps.dp_state, ps.phase)
    fails, _ = _verdict(f"{tag} fp64 oracle", pl64, r.pt64, r.arr64, r.model, r.skip, exact=True, fam=r.fam)
    assert not fails, "\n".join(fails)
    # fp32, end to end: inside every bound and allowed set at f_err = b_F
    fails, jd = _verdict(f"{tag} fp32 oracle end to end", r.pl, r.pt, r.arr32, r.model, r.skip, fam=r.fam)
    PT.report_ambiguous(f"{tag} fp32 oracle end to end", jd, PT.NEAR_MAX, fails)
    assert not fails, "\n".join(fails)
    # fp32, isolated: its elastic twin moves the same way and holds its F_trial; the truth of that exact matrix, f_err = 0
    tw = r.twin32
    assert np.array_equal(tw["pos"], r.arr32["pos"]) and np.array_equal(tw["vel"], r.arr32["vel"])
    pl_iso = PT.Plastic(T.mat(tw["def_grad"], d), None, ps.dp, ps.dp_state, ps.phase)
    fails, jd = _verdict(f"{tag} fp32 oracle isolated", pl_iso, r.pt_iso, r.arr32, r.model, r.skip, F_trial32=tw["def_grad"], fam=r.fam)
    PT.report_ambiguous(f"{tag} fp32 oracle isolated", jd, PT.AMBIGUOUS_MAX, fails)
    same = ~jd.changed & (r.arr32["phase"][:, 0] == ps.phase[:, 0])
    report_margin(f"{tag} fp32 oracle: unprojected and unbroken particles holding the twin's F exactly", int(same.sum()), 0)
    assert same.sum() >= 0.1 * ps.n
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("case,d", CASE_IDS)
def test_the_scenes_meet_their_conditions(oracle_libs, case, d):
    r = _run(case, d)
    counts = PT.conditions(case, r.pl, r.pl_in, int(r.pt.near_cap.sum()))
    for k, v in counts.items():
        report_margin(f"{case} {d}D conditions: {k}", v, 0)
    if r.sc["colliders"]:
        report_margin(f"{case} {d}D conditions: particles with a collider affinity", r.felt, 0)
        assert r.felt > 0.02 * r.ps.n, "the collider is not felt by the cloud"
    gdt = np.linalg.norm(r.pt.grad, axis=(1, 2)) * T.DT
    assert 0.01 <= np.median(gdt) <= 0.03, np.median(gdt)
    # max_stretch inside the window around s_max(F_in); uni_dp 2 has one value
    br = r.pl_in.breakable
    if br.any():
        ratio = r.pl_in.max_stretch[br] / r.pl_in.s_max[br] - 1.0
        assert PT.STRETCH_WINDOW[0] - 1e-6 <= ratio.min() and ratio.max() <= PT.STRETCH_WINDOW[1] + 1e-6
    mode = PT.CASES[case][1]
    assert (len(np.unique(r.ps.phase[:, 1])) == 1) == (mode == 2 or not PT.CASES[case][2])
    # the isolated truth (of the fp32 oracle's twin) under today's cap
    pl_iso = PT.Plastic(T.mat(r.twin32["def_grad"], d), None, r.ps.dp, r.ps.dp_state, r.ps.phase)
    amb, _ = pl_iso.ambiguous()
    assert amb.sum() <= PT.AMBIGUOUS_MAX * r.ps.n, int(amb.sum())


# ------------------------------------------------------------------------------------------------ the widening is a bound
@pytest.mark.parametrize("d", [2, 3])
def test_perturbations_of_the_trial_matrix_stay_inside_the_stated_widening(d):
    rng = np.random.default_rng(40 + d)
    cat = DM.dp_catalogue(d, rng)
    draws = 300
    worst = {}
    for fam, F32 in cat.items():
        F0 = DM.mat(F32, d)
        m = len(F0)
        if m == 0:
            continue
        per = max(1, -(-draws // m))
        F = np.repeat(F0, per, axis=0)
        n = len(F)
        a = np.abs(np.linalg.svd(F, compute_uv=False))
        level = np.where(rng.random(n) < 0.5, 4e-6 * np.linalg.norm(F, axis=(1, 2)), 10.0 ** rng.uniform(-4, -0.5, n) * a.min(1))
        f_err = np.minimum(level, 0.45 * a.min(1))
        dF = rng.normal(size=F.shape)
        dF *= (f_err / np.linalg.norm(dF, axis=(1, 2)))[:, None, None]
        dp = np.tile(np.array([0.61, 0.157, 0.2, 0.1745, 4e5, 4e5]), (n, 1))
        dp[:, 0] *= rng.uniform(0.9, 1.1, n)
        state = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.0, 2.0, n), rng.uniform(-0.2, 0.2, n)], 1)
        state[::2] = (1.0, 1.0, 0.0)
        r0 = DM.dp_outcomes64(dp, state, F, DM.svd_lapack(DM.unmat(F)), f_err)
        r1 = DM.dp_outcomes64(dp, state, F + dF, DM.svd_lapack(DM.unmat(F + dF)))
        assert not r0["amb_input"].any()
        c = np.abs((d * dp[:, 4] + 2.0 * dp[:, 5]) / (2.0 * dp[:, 5]) * DM.dp_alpha64(dp, state[:, 1]))
        s0, s1 = DM.svd_lapack(DM.unmat(F))[1], DM.svd_lapack(DM.unmat(F + dF))[1]
        add = (2.0 * f_err[:, None] / np.abs(s0)).sum(1)
        checks = {"s_max / f_err": (np.abs(s1.max(1) - s0.max(1)), f_err),
                  "trace / strain band": (np.abs(r1["tr"] - r0["tr"]), add),
                  "|dev| / strain band": (np.abs(r1["dev_norm"] - r0["dev_norm"]), add),
                  "gamma / gamma band": (np.abs(r1["gamma"] - r0["gamma"]), add * (1.0 + c))}
        clear_dir = r0["dev_norm"] > 2.0 * add                       # (below, the cone's direction is anyone's: amb_zero)
        for br, sel in (("A", np.ones(n, bool)), ("B", clear_dir), ("N", np.ones(n, bool))):
            o0, o1 = r0["out"][br], r1["out"][br]
            checks[f"{br}: F' / K f_err"] = (np.linalg.norm(o1["F"] - o0["F"], axis=(1, 2))[sel], o0["lip_F"][sel])
            for k in range(3):
                checks[f"{br}: state[{k}] / K f_err"] = (np.abs(o1["state"][:, k] - o0["state"][:, k])[sel], o0["lip_state"][sel, k])
        for name, (val, bound) in checks.items():
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(bound > 0, val / bound, np.where(val > 1e-15, np.inf, 0.0))
            w = float(ratio.max()) if ratio.size else 0.0
            worst[name] = max(worst.get(name, 0.0), w)
            # (1e-6: F + dF is itself rounded, u64 |F| against an f_err of 1e-4 s_min at the least)
            assert w <= 1.0 + 1e-6, f"{d}D {fam}: {name}: {w:.4g} (#{int(np.argmax(ratio))})"
    for name, w in worst.items():
        report_margin(f"Lipschitz self-check {d}D: {name}", w, 1.0)
    # the bound is a bound, not a blanket: the F' of every moving branch uses a good part of it somewhere
    assert worst["A: F' / K f_err"] > 0.2 and worst["B: F' / K f_err"] > 0.05, worst


# ------------------------------------------------------------------------------------------------ deliberate mistakes
MISTAKES = ("fracture tested on F_in", "SVD of F_in used for the stress", "st[1] overwritten instead of accumulated",
            "st[2] with the opposite sign", "st[0] not scaled by prev_det / new_det",
            "projection skipped for particles that broke in this substep", "plastic state taken from particle i + 1",
            "plastic state taken from particle i - 1", "uniform max_stretch used where it differs per particle")


def _restate(r: Run, mistake=None):
    """the update in numpy, fp64, from the truth's trial state; `mistake`: one of MISTAKES made on purpose"""
    ps, inp, pt, d = r.ps, r.inp, r.pt, r.d
    f = lambda a: np.asarray(a, np.float64)
    dp, st_own, ph = f(ps.dp), f(ps.dp_state), f(ps.phase)
    ms = ph[:, 1].copy()
    if mistake == MISTAKES[8]:
        ms[:] = ms[0]
    st_in = st_own
    if mistake in MISTAKES[6:8]:
        st_in = np.roll(st_own, -1 if mistake == MISTAKES[6] else 1, axis=0)
    F_tr = pt.F
    s = np.linalg.svd(inp.F if mistake == MISTAKES[0] else F_tr, compute_uv=False)
    breakable = (ph[:, 0] > 0) & (ms > 0)
    broken = breakable & (s.max(1) > ms)
    phase = np.where(broken, 0.0, ph[:, 0])
    cand = (phase == 0.0) & (dp[:, 4] != 0.0)
    if mistake == MISTAKES[5]:
        cand &= ~broken
    F_out, st_out = F_tr.copy(), st_own.copy()
    idx = np.nonzero(cand)[0]
    Fp, stp = np_oracle.drucker_prager_project(dp[idx], st_in[idx], F_tr[idx])
    moved = ~(np.all(stp == st_in[idx], axis=1) & np.all(Fp == F_tr[idx], axis=(1, 2)))
    if mistake == MISTAKES[2]:
        stp[:, 1] = stp[:, 1] - st_in[idx, 1]
    if mistake == MISTAKES[3]:
        stp[:, 2] = st_in[idx, 2] - (stp[:, 2] - st_in[idx, 2])
    if mistake == MISTAKES[4]:
        stp[:, 0] = st_in[idx, 0]
    F_out[idx[moved]], st_out[idx[moved]] = Fp[moved], stp[moved]
    if r.model == 0:
        U, sv, _ = DM.svd_lapack(DM.unmat(inp.F if mistake == MISTAKES[1] else F_out))
        tau = DM.tau_corotated64(F_out, inp.lam, inp.mu, U, sv)
    else:
        tau = DM.tau_neo_hookean64(F_out, inp.lam, inp.mu)
    Cn = pt.grad * inp.m[:, None, None] - tau * (inp.vol * pt.invd * pt.dt)[:, None, None]
    return dict(pos=pt.x, vel=pt.vel, def_grad=DM.unmat(F_out), affine=DM.unmat(Cn), dp_state=st_out,
                phase=np.stack([phase, ph[:, 1]], 1))


_CHECKS = (("phase is not", "fracture decision"), ("plastic state changed", "state without projection"), ("projection candidates off", "branch / F' / dp_state"),
           (": x (", "x"), (": v (", "v"), (": F (", "F of the unprojected"), (": C' (", "C'"))


def _what(line):
    """the check a failure line names, without the scene and the counts"""
    return next((name for key, name in _CHECKS if key in line), line[:60])


def test_deliberate_mistakes_break_a_bound_or_a_decision(oracle_libs, monkeypatch):
    caught = {m: {} for m in MISTAKES}
    with monkeypatch.context() as mp:          # (verdicts on wrong results are no margins: nothing of them is recorded)
        for mod in (T, DM, PT):
            mp.setattr(mod, "report_margin", lambda *a, **k: None)
        for case, d in CASE_IDS:
            r = _run(case, d)
            fails, _ = _verdict(f"{case} {d}D restated", r.pl, r.pt, _restate(r), r.model, r.skip)
            assert not fails, "the restatement itself is off:\n" + "\n".join(fails)
            for m in MISTAKES:
                fails, jd = _verdict(f"{case} {d}D with: {m}", r.pl, r.pt, _restate(r, m), r.model, r.skip)
                if fails:
                    caught[m][f"{case} {d}D"] = sorted({_what(x) for x in fails})
    for m in MISTAKES:
        broke = sorted({w for v in caught[m].values() for w in v})
        report_margin(f"deliberate mistake '{m}': scenes on which it breaks a check", len(caught[m]), 0, of=len(CASE_IDS), breaks=", ".join(broke))
    missed = [m for m in MISTAKES if not caught[m]]
    assert not missed, "no bound and no decision notices the mistake: " + "; ".join(missed)


# ------------------------------------------------------------------------------------------------ steady state and slabs
def _as_particles(ps, arr):
    """the ParticleSet of an oracle state (fp32 arrays of its `arr`)"""
    out = ps.copy()
    for k in ("pos", "vel", "def_grad", "affine", "dp_state", "phase"):
        getattr(out, k)[:] = arr[k]
    return out


@pytest.mark.parametrize("case,d,h", PT.STEADY)
def test_the_steady_state_scenes_meet_their_conditions_and_the_fp32_oracle_fits(oracle_libs, case, d, h):
    """15 substeps of the C fp32 oracle, its 16th judged like a kernel's: inside every bound, and the state it runs on holds
    what the GPU test asserts of its own run: cell changers, particles projected before and again, particles that change cell and
    are projected in the same substep, the caps."""
    sc, fam = PT.scene(case, d, h=h, steady=True)
    ps = sc["particles"]
    st32 = run_oracle(sc, 15, np.float32)
    before = _as_particles(ps, st32.arr)
    st32.step(1)
    got = {k: v.copy() for k, v in st32.arr.items()}
    now = dict(sc, particles=before)
    twin = run_oracle(PT.strip(now), 1, np.float32).arr
    inp = T.Inputs.of(before)
    _, _, pt = T.substep(inp, h, T.DT, sc["params"].gravity)
    tag = f"steady state {case} {d}D fp32 oracle"
    assert np.array_equal(twin["pos"], got["pos"]) and np.array_equal(twin["vel"], got["vel"])
    pl = PT.Plastic(pt.F, pt.b_F, before.dp, before.dp_state, before.phase)
    fails, jd = _verdict(f"{tag} end to end", pl, pt, got, sc["model"], fam=fam)
    PT.report_ambiguous(f"{tag} end to end", jd, PT.NEAR_MAX, fails)
    pl_iso = PT.Plastic(T.mat(twin["def_grad"], d), None, before.dp, before.dp_state, before.phase)
    jd_iso = PT.judge(f"{tag} isolated", pl_iso, got, fails, F_trial32=twin["def_grad"], fam=fam)
    PT.report_ambiguous(f"{tag} isolated", jd_iso, PT.AMBIGUOUS_MAX, fails)
    assert not fails, "\n".join(fails)
    amb, pure = pl.ambiguous()
    counts = dict(ambiguous=int(amb.sum()), isotropic_ambiguous=int(pure.sum()), near_cap=int(pt.near_cap.sum()),
                  **{br: int((jd_iso.branch == br).sum()) for br in "ABN"})
    assert amb.sum() <= PT.NEAR_MAX * ps.n and pt.near_cap.sum() <= PT.NEAR_MAX * ps.n, counts
    again = jd_iso.changed & np.any(before.dp_state != np.array([1.0, 1.0, 0.0], np.float32), axis=1)
    moved = np.any(T.assoc_cell(before.pos, h) != T.assoc_cell(got["pos"].astype(np.float32), h), axis=1)
    same = ~jd_iso.changed & (got["phase"][:, 0] == before.phase[:, 0])
    counts.update(projected_again=int(again.sum()), moved_and_projected=int((moved & jd_iso.changed).sum()), cell_changers=int(moved.sum()),
                  unprojected_unbroken=int(same.sum()))
    for k, v in counts.items():
        report_margin(f"{tag} conditions: {k}", v, 0)
    assert counts["projected_again"] >= 20 and counts["moved_and_projected"] >= 20 and counts["unprojected_unbroken"] >= 0.1 * ps.n, counts


@pytest.mark.parametrize("world,d,h", [(2, 3, 0.5), (3, 2, 0.3)])
def test_the_slab_scenes_meet_their_conditions_and_the_fp32_oracle_fits(oracle_libs, world, d, h):
    """The drifting plastic clusters of the slab test as ONE domain through the C fp32 oracle: its substeps 2 .. 7 inside every
    bound at extra_levels = 8, and enough arrivals (particles whose block left the range of the rank that held them: the owner of
    their block one substep earlier) that are projected or break in the substep they arrive in."""
    from test_gpu_plastic_motion import drifting_plastic
    from wgsparkl_amd.sharded import SlabPartition, associated_block_x
    sc = drifting_plastic(d, h, world)
    ps = sc["particles"]
    part = SlabPartition.balanced(associated_block_x(ps.pos, h, d), world)
    lo_hi = np.array([part.block_range(r) for r in range(world)])
    holder = part.owner_of_blocks(associated_block_x(ps.pos, h, d))
    st32 = run_oracle(sc, 1, np.float32)
    n_arr = n_plastic = 0
    fails = []
    for step in range(6):
        pre = {k: v.copy() for k, v in st32.arr.items()}
        st32.step(1)
        post = st32.arr
        inp = T.Inputs.of(pre)
        bx = associated_block_x(inp.pos32, h, d)
        arrival = (bx < lo_hi[holder, 0]) | (bx >= lo_hi[holder, 1])
        _, _, pt = T.substep(inp, h, T.DT, sc["params"].gravity, extra_levels=8.0)
        pl = PT.Plastic(pt.F, pt.b_F, pre["dp"], pre["dp_state"], pre["phase"])
        f, jd = _verdict(f"plastic slabs {world}x {d}D substep {step} fp32 oracle", pl, pt, post, sc["model"])
        PT.report_ambiguous(f"plastic slabs {world}x {d}D substep {step} fp32 oracle", jd, PT.NEAR_MAX, f)
        fails += f
        assert pt.near_cap.sum() <= PT.NEAR_MAX * ps.n
        broke = (post["phase"][:, 0] == 0) & (pre["phase"][:, 0] != 0)
        n_arr += int(arrival.sum())
        n_plastic += int((arrival & (jd.changed | broke)).sum())
        holder = part.owner_of_blocks(bx)
    report_margin(f"plastic slabs {world}x {d}D fp32 oracle: arrivals", n_arr, 0)
    report_margin(f"plastic slabs {world}x {d}D fp32 oracle: arrivals projected or broken in the substep they arrive in", n_plastic, 0)
    assert not fails, "\n".join(fails)
    assert n_arr >= 20 and n_plastic >= 5, (n_arr, n_plastic)
