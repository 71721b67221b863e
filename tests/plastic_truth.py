"""fp64 truth of the plastic particle update IN MOTION (wgsparkl_amd/csrc/g2p_body.inc, and its second copy in arrivals_body.inc):
F_trial = F + (grad dt) F, the fracture test, the Drucker-Prager projection and the stress, all inside one substep. Shared by
tests/test_plastic_truth.py (CPU: the truth against the C fp64 oracle, the bounds against the C fp32 oracle, against
perturbations and against deliberate mistakes) and tests/test_gpu_plastic_motion.py (the HIP kernels per particle).

It composes the two truths the suite already trusts and restates neither:
- the trial state: transfer_truth.substep / isolated (or cpic_truth.substep with a collider) give x, v, grad and
  F_trial = pt.F in fp64 from the fp32 inputs, with their bounds; b_F is the normwise (Frobenius) bound of a kernel's F_trial;
- decisions and outcomes: evaluated on F_trial, never on F_in. Fracture by the rule of test_gpu_constitutive (breakable:
  phase > 0 and max_stretch > 0; broken: s_max > max_stretch), then Drucker-Prager for phase == 0 and dp[4] != 0 through
  devmath_truth.dp_outcomes64 / dp_allowed / dp_match.

The one thing that is new is that the matrix the kernel decides on and projects is not the truth's: it is the kernel's own
fp32 F_trial, within f_err = b_F of pt.F. devmath_truth.dp_outcomes64 takes that `f_err` and widens its bands and its outcome
tolerances (derivation in its docstring); the fracture band widens by Weyl's inequality, |s_max(F + dF) - s_max(F)| <= |dF|:
    |s_max - max_stretch| <= C_DEC u s_max + f_err        (either decision is then a legitimate one).
Two ways to judge a run follow:
- isolated: the same scene stripped of plasticity (`strip`) gives the kernel's own F_trial32 bit for bit (P2G does not read
  the plastic state). The truth is then taken of that exact fp32 matrix, f_err = 0: the tight bands of devmath_truth;
- end to end: the truth of pt.F with f_err = b_F.
The stress keeps transfer_truth's rule: C' from tau in fp64 of the F the kernel produced (check_particles), for a projected
corotated particle the stress of the projected F.

`scene` builds the moving plastic scenes both test files run (`CASES`); `Plastic` is the truth, `judge` the per-particle
verdict on a result (a kernel's, or the C oracle's). The fracture decision (`Fracture`) and what a judge asks of the particles that
were not projected (`gate`) do not depend on the plasticity rule: tests/snow_truth.py uses the same two."""
from typing import NamedTuple

import numpy as np

import devmath_truth as DM
import transfer_truth as T
from helpers import report_margin

U32, U64 = T.U32, T.U64
AMBIGUOUS_MAX = 0.02     # decision-ambiguous particles outside isotropic strain, isolated check (test_gpu_constitutive's cap)
NEAR_MAX = 0.05          # ... end to end (the bands carry f_err), and particles near the speed cap
STRETCH_WINDOW = (-0.01, 0.03)   # max_stretch / s_max(F_in) - 1 of a breakable particle: the substep's motion decides

CASES = {
    # name: (model, uni_dp mode the library will pick, fracture, per-particle mass / material, WGS_DEBUG switch, collider)
    "mode2_corotated": (0, 2, False, True, None, False),
    "mode2_fracture_neo_hookean": (1, 2, True, True, None, False),
    "mode2_fracture_uniform_material": (0, 2, True, False, None, False),      # 3D: mass and material are kernel arguments
    "mode1_fracture_corotated": (0, 1, True, True, None, False),
    "mode1_neo_hookean": (1, 1, False, True, None, False),
    "mode0_per_particle_state_fracture": (0, 0, True, True, None, False),
    "forced_mode0_fracture": (0, 2, True, False, "NO_UNIFORM", False),
    "mode2_fracture_two_pass": (0, 2, True, False, "G2P_TWO_PASSES", False),
    "mode1_fracture_collider": (0, 1, True, True, None, True),
}
UNIFORM_MAX_STRETCH = 1.25
# The steady-state scenes (case, d, h): 15 substeps, the 16th checked; every uni_dp layout, both dimensions. h = 0.5 only: a
# particle that was projected sits ON the yield surface (gamma = 0), and the next substep moves it by dt |grad| ~ 0.015. At
# h = 0.3 b_F carries the weights' 2 |cell| u (transfer_truth.Stencil.weight_error) times |v| and the end-to-end band of gamma is
# as wide as that motion: a quarter of the particles would be decision-ambiguous, against the cap of NEAR_MAX (measured with the
# truth alone, tests/test_plastic_truth.py). A power of two keeps cell * h exact and the band a fifth as wide.
STEADY = [("mode0_per_particle_state_fracture", 3, 0.5), ("mode1_fracture_corotated", 2, 0.5), ("mode2_fracture_neo_hookean", 3, 0.5),
          ("mode2_corotated", 2, 0.5)]
# The slab scenes drift at 0.6 h / dt: b_F, which grows with |v|, is wider still (a third of the plastic particles are ambiguous
# end to end), and the cap is on the share of ALL particles: only the leading SLAB_LEAD cells of the clusters that cross a cut, the
# particles that arrive on another rank within the checked substeps, are plastic or breakable; the others are elastic.
SLAB_LEAD = 3.0
# The same reason decides h of the one-substep scenes: 0.3 in 2D and 0.5 in 3D. In 3D at h = 0.3 six to nine per cent of the
# particles are ambiguous end to end, over the cap; in 2D three to four.
H_OF = {2: 0.3, 3: 0.5}


# ------------------------------------------------------------------------------------------------ scenes
def _s_max(F32, d):
    return DM.svd_lapack(F32)[1].max(1)


def _draw(cat, n, rng):
    F = np.concatenate(list(cat.values()))
    fam = np.concatenate([[k] * len(v) for k, v in cat.items()])
    idx = np.concatenate([np.arange(len(F)), rng.integers(0, len(F), max(0, n - len(F)))])[:n]
    idx = rng.permutation(idx)
    return F[idx].copy(), fam[idx]


def velocity_field(pos, h, rng, rate=1.0):
    """(vel [n, d], A [d, d]): v = A (x - c) + noise with A a swirl plus a stretching part, |A| dt ~ 0.025 * rate"""
    n, d = pos.shape
    A = np.zeros((d, d))
    A[0, 1], A[1, 0] = -12.0, 12.0
    A += np.diag([10.0, -14.0, 6.0][:d])
    if d == 3:
        A[2, 0], A[1, 2] = 5.0, -4.0
    A *= rate
    c = pos.mean(0)
    return (pos - c) @ A.T + rng.normal(0.0, 2.0 * h * rate, (n, d)), A


def scene(case, d, h=None, seed=0, steady=False, n=None, pos=None, vel=None, elastic=None):
    """(scene dict, family name per particle). A block of particles about 3 blocks wide (test_gpu_transfer._moving) in the
    velocity field above, T.DT and T.GRAVITY; F from devmath_truth.dp_catalogue (breakable particles: the moderate families
    of `catalogue`), max_stretch of every breakable particle inside s_max(F_in) * (1 + STRETCH_WINDOW). In a fracture case
    every other particle is breakable (phase 1), the rest plastic from the start (phase 0); without fracture all are phase 0.
    uni_dp 2 needs ONE max_stretch: there F_in of a breakable particle is scaled to put its s_max in the window instead.
    `steady`: deformations near I (log s ~ N(-0.01 or -0.06, 0.03): on the cone and inside it) and a softer material, so that 16
    substeps stay below the speed cap. `elastic`: the share of particles that are neither plastic nor about to break (phase 1,
    max_stretch -1; under uni_dp 2 the one max_stretch, which a deformation near I does not reach), or a mask of them; default 0.25 in a steady scene
    (a particle that is projected once is projected in most later substeps: without them nothing is left unprojected), else 0.
    `pos`, `vel`: given positions and velocities (the slab scenes) in place of the block."""
    from wgsparkl_amd.models import DruckerPrager
    model, mode, fracture, per_particle, _, collider = CASES[case]
    h = H_OF[d] if h is None else h
    rng = np.random.default_rng(7000 + 31 * seed + 7 * d + sorted(CASES).index(case))
    bw = T.bw_of(d)
    if pos is None:
        n = n or (3000 if d == 3 else 1500)
        pos = rng.uniform(2 * bw * h, 5 * bw * h, (n, d))
    n = len(pos)
    pos32 = np.asarray(pos, np.float32)
    v, A = velocity_field(pos32.astype(np.float64), h, rng, rate=0.6 if steady else 1.0)
    sc = T._finish(pos32, h, rng, vel=v if vel is None else vel, uniform=not per_particle, model=model)
    ps = sc["particles"]
    ps.affine[:] = ((T.unmat(A[None])[0][None, :] + rng.normal(0.0, 2.0, (n, d * d))) * ps.mass[:, None]).astype(np.float32)
    # ---- deformation gradients
    elastic = (0.25 if steady else 0.0) if elastic is None else elastic
    assert steady or not (np.any(elastic) and mode == 2 and fracture)
    order = rng.permutation(n)
    is_elastic, breakable = np.zeros(n, bool), np.zeros(n, bool)
    if np.ndim(elastic):                               # a mask: these particles
        is_elastic[:] = elastic
        order = np.concatenate([order[is_elastic[order]], order[~is_elastic[order]]])
    else:
        is_elastic[order[: int(elastic * n)]] = True
    if fracture:
        breakable[order[int(is_elastic.sum()):][::2]] = True
    if steady:
        s = np.exp(rng.normal(np.where(rng.random(n) < 0.5, -0.01, -0.06)[:, None], 0.03, (n, d)))
        F = T.unmat(DM._usv(rng, s)).astype(np.float32)
        fam = np.full(n, "near_identity")
        for k in ("lambda_", "mu"):
            getattr(ps, k)[:] *= np.float32(0.1)
    else:
        F, fam = _draw(DM.dp_catalogue(d, rng), n, rng)
        cat = DM.catalogue(d, seed=5)
        Fb, famb = _draw({k: v for k, v in cat.items() if k == "well_conditioned" or k.startswith("clustered")}, n, rng)
        F[breakable], fam[breakable] = Fb[breakable], famb[breakable]
    # ---- plasticity and phase
    dp = DruckerPrager.new(1e6, 0.25).as_array()
    ps.dp[:] = dp
    ps.has_plasticity[:] = True
    ps.has_phase[:] = True
    delta = rng.uniform(*STRETCH_WINDOW, n)
    if mode == 2:
        # (1.25, not 1: scaled to s_max ~ 1 the clustered families sit on EVERY threshold at once — trace, |dev| and gamma all ~ 0)
        ms = np.full(n, UNIFORM_MAX_STRETCH, np.float32)
        scale = (UNIFORM_MAX_STRETCH / (1.0 + delta)) / _s_max(F, d)
        F[breakable] = (F[breakable] * scale[breakable, None]).astype(np.float32)
    else:
        ms = (_s_max(F, d) * (1.0 + delta)).astype(np.float32)
        alt = DruckerPrager.new(3e5, 0.3).as_array()
        ps.dp[::3, 4:6] = alt[4:6]
    if mode == 0:
        ps.dp[:, 0] = (ps.dp[:, 0] * rng.uniform(0.9, 1.1, n)).astype(np.float32)
        ps.dp_state[:] = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.0, 2.0, n), rng.uniform(-0.2, 0.2, n)], 1).astype(np.float32)
    ps.def_grad[:] = F
    ps.phase[:, 0] = np.where(breakable | is_elastic, 1.0, 0.0).astype(np.float32)
    ps.phase[:, 1] = np.where(is_elastic & (mode != 2), np.float32(-1.0), ms) if fracture else np.float32(-1.0)
    if collider:
        from wgsparkl_amd.solver import Collider
        r = 4.0 * bw * h                                # (wide: its cap lies within two cells of most of the cloud's top)
        c = np.full(d, 3.5 * bw * h)
        c[1] = 5 * bw * h + r + 0.3 * h                 # its surface a third of a cell above the top of the cloud: nothing inside
        sc["colliders"] = [Collider.ball(float(np.float32(r)), tuple(float(x) for x in c.astype(np.float32)))]
        sc["grid_capacity"] = max(sc["grid_capacity"], 1024)
    return sc, fam


def strip(sc, particles=None):
    """the elastic twin of a scene (or of a read-back state of it): phase (1, -1) and no plasticity. P2G, the grid update and
    G2P do not read the plastic state, so its x and v are the plastic run's and its def_grad is the F_trial of that run."""
    ps = (sc["particles"] if particles is None else particles).copy()
    from wgsparkl_amd.models import DruckerPrager
    ps.dp[:] = DruckerPrager.new(-1.0, -1.0).as_array()
    ps.dp_state[:] = np.array([1.0, 1.0, 0.0], np.float32)
    ps.phase[:] = np.array([1.0, -1.0], np.float32)
    ps.has_plasticity = np.zeros(ps.n, bool)
    ps.has_phase = np.ones(ps.n, bool)
    return dict(sc, particles=ps)


# ------------------------------------------------------------------------------------------------ the truth
class Fracture:
    """The fp64 fracture decision on a trial deformation gradient, whatever plasticity rule follows it.

    F [n, d, d] float64, f_err [n] its normwise bound (None: exact), phase [n, 2] the fp32 input of the substep. breakable: phase > 0
    and max_stretch > 0; broken: s_max > max_stretch; inside the band `amb_frac` either decision is a legitimate one."""

    def __init__(self, F, f_err, phase):
        F = np.asarray(F, np.float64)
        self.n, self.d = F.shape[0], F.shape[1]
        self.f_err = np.zeros(self.n) if f_err is None else np.asarray(f_err, np.float64)
        ph = np.asarray(phase, np.float32).astype(np.float64)
        self.svd = DM.svd_lapack(T.unmat(F))
        s = self.svd[1]
        _, smax, _ = DM.sv_stats(s)
        self.phase_in, self.max_stretch = ph[:, 0], ph[:, 1]
        self.breakable = (self.phase_in > 0) & (self.max_stretch > 0)
        self.s_max = s.max(1)
        self.broken = self.breakable & (self.s_max > self.max_stretch)
        self.amb_frac = self.breakable & (np.abs(self.s_max - self.max_stretch) <= DM.C_DEC * U32 * smax + self.f_err)
        self.phase64 = np.where(self.broken, 0.0, self.phase_in)


class Plastic:
    """fp64 fracture and Drucker-Prager decisions and outcomes on a trial deformation gradient.

    F [n, d, d] float64 (transfer_truth's pt.F, or an exact fp32 matrix), f_err [n] its normwise bound (None: exact);
    dp [n, 6], state [n, 3], phase [n, 2]: the fp32 inputs of the substep."""

    def __init__(self, F, f_err, dp, state, phase):
        F = np.asarray(F, np.float64)
        self.F = F
        self.fr = fr = Fracture(F, f_err, phase)
        for k in ("n", "d", "f_err", "svd", "s_max", "phase_in", "max_stretch", "breakable", "broken", "amb_frac", "phase64"):
            setattr(self, k, getattr(fr, k))
        self.dp32, self.state32 = np.asarray(dp, np.float32), np.asarray(state, np.float32)
        self.dp, self.state = self.dp32.astype(np.float64), self.state32.astype(np.float64)
        self.has_dp = self.dp[:, 4] != 0.0
        self.cand64 = (self.phase64 == 0.0) & self.has_dp
        self.res = DM.dp_outcomes64(self.dp, self.state, F, self.svd, f_err)
        self.allowed = DM.dp_allowed(self.res)
        self.fnorm = np.linalg.norm(F, axis=(1, 2))
        # one label per particle: '-' no projection attempted, else the branch fp64 takes
        self.label = np.where(self.cand64, self.res["branch"], "-")
        self.multi = np.array([len(a) > 1 for a in self.allowed])

    def ambiguous(self, cand=None):
        """(ambiguous outside isotropic strain, ambiguous in isotropic strain) over the candidates `cand` (default: the fp64 ones,
        and every breakable particle inside the fracture band: broken it is a candidate)"""
        cand = (self.cand64 | (self.amb_frac & self.has_dp)) if cand is None else cand
        amb = self.amb_frac | (cand & self.multi)
        pure = cand & self.res["amb_zero"]
        return amb & ~pure, amb & pure


class Judged(NamedTuple):
    cand: np.ndarray        # [n] projection attempted by the judged run (its own phase == 0, dp[4] != 0)
    changed: np.ndarray     # [n] ... and done: F or the state moved
    branch: np.ndarray      # [n] '-' (no candidate), the matched branch, or '?' (none matched)
    ratio: np.ndarray       # [n] worst error / bound of the matched branch (0 where not a candidate)
    bad: np.ndarray         # [n] any complaint
    amb: np.ndarray         # [n] decision-ambiguous outside isotropic strain
    pure: np.ndarray        # [n] ... in isotropic strain


def _get(got):
    return (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))


class Gate(NamedTuple):
    cand: np.ndarray        # [n] the judged run's own gate: its phase == 0 and the particle's switch on
    changed: np.ndarray     # [n] the plastic state moved or (with F_trial32) F is not the twin's
    bad: np.ndarray         # [n] any complaint so far; `complain` goes on marking it
    complain: object        # complain(mask, what): marks `bad` and appends one line to `fails`


def gate(tag, fr: Fracture, has, state32, got, fails, F_trial32=None, exact=False, name=None):
    """What every plasticity rule's judge asks first of a run (ParticleSet or dict), with `has` the particles' switch (dp[4] != 0) and
    `state32` their plastic state before the substep:
    - phase[:, 1] is bit-unchanged; phase[:, 0] is the fp64 decision of `fr` outside its band, inside it the old value or 0 (`exact`: no band);
    - a particle the run did not send through the projection (its phase != 0 or the switch off) keeps its state bit for bit and, with
      `F_trial32` (the twin's def_grad: the run's own F_trial), holds exactly that matrix."""
    g = _get(got)
    n = fr.n
    name = name or (lambda i: f"#{i}")
    bad = np.zeros(n, bool)

    def complain(mask, what):
        if mask.any():
            bad[mask] = True
            fails.append(f"{tag}: {what}: {int(mask.sum())} particles (first {name(int(np.argmax(mask)))})")

    ph = np.asarray(g("phase"), np.float64)
    complain(ph[:, 1] != fr.max_stretch, "max_stretch changed")
    phase = ph[:, 0]
    legit = (phase == fr.phase_in) | (fr.breakable & (phase == 0.0))
    band = np.zeros(n, bool) if exact else fr.amb_frac
    complain(~legit | ((phase != fr.phase64) & ~band), "phase is not the fp64 fracture decision on F_trial")
    cand = (phase == 0.0) & has
    st_moved = ~np.all(np.asarray(g("dp_state")) == state32, axis=1)
    changed = st_moved.copy()
    if F_trial32 is not None:
        changed |= ~np.all(np.asarray(g("def_grad")) == np.asarray(F_trial32), axis=1)
    complain(~cand & st_moved, "plastic state changed without a projection")
    if F_trial32 is not None:
        complain(~cand & changed, "F is not the elastic twin's F_trial although no projection was attempted")
    return Gate(cand, changed, bad, complain)


def judge(tag, pl: Plastic, got, fails, F_trial32=None, exact=False, fam=None):
    """Every particle's phase, def_grad and dp_state of a run against the truth `pl`.
    - phase, and the state and F of a particle the run did not attempt to project: `gate`;
    - one it did attempt is matched against the allowed branches (devmath_truth.dp_match). "Projected" is read off the state (it moved),
      and with `F_trial32` (the twin's def_grad: the run's own F_trial) also off F: an unprojected particle then holds exactly
      F_trial32, which is asserted;
    - `exact` (an fp64 run against the fp64 truth): the fp64 decisions themselves, no band, and every error within
      C u64 of the scales instead of C u32.
    F of the particles that were not projected is the caller's (transfer_truth.check_particles with own_F = changed)."""
    g = _get(got)
    n, d = pl.n, pl.d
    F_out = T.mat(np.asarray(g("def_grad"), np.float64), d)
    st_out = np.asarray(g("dp_state"))
    name = (lambda i: f"#{i}" + (f" ({fam[i]})" if fam is not None else ""))
    cand, changed, bad, _ = gate(tag, pl.fr, pl.has_dp, pl.state32, got, fails, F_trial32, exact, name)
    branch = np.full(n, "-", dtype="<U1")
    ratio = np.zeros(n)
    lines = []
    for i in np.nonzero(cand)[0]:
        br, w = DM.dp_match(pl.res, i, changed[i], F_out[i], st_out[i].astype(np.float64), pl.fnorm[i])
        if exact and br is not None and (br != pl.res["branch"][i] or not w <= U64 / U32):
            br = None
        if br is None or not w <= 1.0:
            bad[i] = True
            branch[i] = "?"
            ratio[i] = w if np.isfinite(w) else np.inf
            lines.append(f"{name(i)}: changed={bool(changed[i])} matches none of {sorted(pl.allowed[i])} (best {br}: {w:.3g} x bound; fp64 "
                         f"branch {pl.res['branch'][i]}, trace {pl.res['tr'][i]:.3e}, gamma {pl.res['gamma'][i]:.3e})")
        else:
            branch[i], ratio[i] = br, w
    ok = cand & (branch != "?")
    report_margin(f"{tag}: Drucker-Prager F / state, worst error / bound (branch-matched)", float(ratio[ok].max()) if ok.any() else 0.0,
                  U64 / U32 if exact else 1.0, n=int(cand.sum()), failures=len(lines))
    if lines:
        fails.append(f"{tag}: {len(lines)} of {int(cand.sum())} projection candidates off:\n  " + "\n  ".join(lines[:8]))
    amb, pure = pl.ambiguous(cand | (pl.amb_frac & pl.has_dp))
    return Judged(cand, changed, branch, ratio, bad, amb, pure)


def report_ambiguous(tag, jd: Judged, cap, fails):
    n = len(jd.cand)
    frac = float(jd.amb.sum()) / n
    report_margin(f"{tag}: decision-ambiguous particles outside isotropic strain (fraction)", frac, cap, count=int(jd.amb.sum()),
                  isotropic_ambiguous=int(jd.pure.sum()))
    if not frac <= cap:
        fails.append(f"{tag}: {int(jd.amb.sum())} of {n} particles are decision-ambiguous outside isotropic strain (cap {cap})")


def conditions(case, pl_trial: Plastic, pl_in: Plastic, near_cap, single_domain=True):
    """The conditions a scene is built for, from the truth alone (pl_trial: end to end, f_err = b_F; pl_in: the same decisions
    taken on F_in). Returns the counts; raises where one is not met."""
    n = pl_trial.n
    fracture = CASES[case][2]
    amb, pure = pl_trial.ambiguous()
    differs = (pl_trial.label != pl_in.label) | (pl_trial.broken != pl_in.broken)
    clear = differs & ~amb & ~pure
    counts = dict(n=n, ambiguous=int(amb.sum()), isotropic_ambiguous=int(pure.sum()), near_cap=int(near_cap),
                  broken=int(pl_trial.broken.sum()), breakable=int(pl_trial.breakable.sum()),
                  decision_differs_from_F_in=int(clear.sum()), **{br: int((pl_trial.label == br).sum()) for br in "ABN"})
    assert amb.sum() <= NEAR_MAX * n, (case, counts)
    assert near_cap <= NEAR_MAX * n, (case, counts)
    if fracture:
        assert 0 < counts["broken"] < counts["breakable"], (case, counts)
        assert counts["decision_differs_from_F_in"] >= 20, (case, counts)
        assert min(counts[br] for br in "ABN") >= (10 if single_domain else 1), (case, counts)
    return counts
