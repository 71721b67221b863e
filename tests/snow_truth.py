"""fp64 truth of the SNOW plastic update (include/wgsparkl_hip.h; wgsparkl_amd/csrc/device_math.h snow_project,
the MODEL 4 instantiations of g2p_body.inc), inside one substep. Shared by tests/test_snow_truth.py (CPU: the truth's own
properties, deliberate mistakes against the judge, the scenes' conditions) and tests/test_gpu_snow.py (the HIP kernels per particle).

It composes the truths the suite already trusts and restates none of them:
- the trial state: transfer_truth.substep / isolated (cpic_truth.substep with a collider) give x, v, grad and F_trial with their
  bounds, as for plastic_truth. The primary check is plastic_truth's isolated one: the scene stripped of plasticity
  (plastic_truth.strip) leaves the kernel's own fp32 F_trial in the twin's def_grad bit for bit, and the truth is taken of that
  exact matrix;
- the fracture decision: plastic_truth.Fracture on that matrix — breakable, broken, its band `amb_frac` and its caps, unchanged;
- the SVD and the stress: devmath_truth.svd_lapack (U, V proper, the sign on the smallest value) and tau_corotated64.

The rule itself, in fp64, for a particle that passes the gate (phase == 0 after the fracture test, dp[4] != 0), with
theta_c = dp[0], theta_s = dp[1], xi = dp[2], cap = dp[3], Jp = state[0] and s the signed singular values of F_trial:
    s^  = clip(s, 1 - theta_c, 1 + theta_s)        Jp' = Jp prod |s| / prod s^        F_E = U diag(s^) V^T
    hf  = exp(min(xi (1 - Jp'), cap))              tau = tau_corotated64(F_E, lambda hf, mu hf)
state[1], state[2] and (lambda, mu) are stored bit for bit; every other particle is the elastic corotated one.

Bounds, each devmath_truth's constant as it stands times what it bounds (u = 2^-24; s_max = max |s|, `sv` = C_SV u s_max the error
of one fp32 singular value; nothing here was fitted to a kernel):
- s^ (read off the stored F_E as its singular values, all positive since 1 - theta_c > 0): clip is monotone and 1-Lipschitz, so the
  sorted clamped values move by no more than the singular values, C_SV u s_max; the stored matrix is U diag(s^) V^T evaluated in
  fp32, C_REC u |F_E| off the exact product, and by Weyl its singular values by no more than that:
      |sort s^_got - sort s^| <= C_SV u s_max + C_REC u |F_E|.
- Jp': prod |s| carries sum_k sv prod_{j != k} |s_j| ABSOLUTE (relative it is unbounded as s_k -> 0, and at the cutoff the kernel's
  s_k is 0: Jp' = 0 is then inside the bound), prod s^ carries sum_k sv / s^_k relative (s^_k >= 1 - theta_c), the two products and
  the quotient a few u each:
      b_Jp = C_DP u |Jp| (sum_k s_max prod_{j != k} |s_j| + prod |s| (d + 2 + sum_k s_max / s^_k)) / prod s^.
- hf: e = min(xi (1 - Jp'), cap) is 1-Lipschitz in its first argument, so |de| <= |xi| b_Jp + C_DP u |e| (the product and the
  difference), and exp carries it relative: b_hf = hf (|xi| b_Jp + C_DP u (|e| + 1)).
- F_E, normwise: F_E = sum_k s^_k u_k v_k^T. V is a product of rotations; column k of U is a rotated column of F over its norm s_k,
  so its direction carries u s_max / |s_k| (devmath_truth.check_svd: the left vectors' bound). In F = sum s_k u_k v_k^T that error
  is multiplied by s_k and is harmless; here it is multiplied by s^_k: the term C_VEC u s_max s^_k / |s_k| — the factor s^ / |s_min|
  by which the map F -> U clip(S) V^T stops being Lipschitz at s_min = 0, where the direction the clamp pushes in is arbitrary. The
  same holds for an inverted matrix whose two smallest |s| are tied: WHICH direction carries the sign is decided by the gap
  |s_(d-1)| - |s_d|, the term C_VEC u s_max (s^_(d-1) + s^_d) / gap. With the reconstruction itself:
      b_FE = C_REC u (|F| + |F_E|) + C_VEC u s_max (sum_k s^_k / |s_k| [+ (s^_(d-1) + s^_d) / gap if s_min < sv]).
  Where one of the ANGLES behind that bound, C_VEC u s_max / |s_k| or C_VEC u s_max / gap, reaches devmath_truth.VEC_MAX_BOUND the
  direction says nothing (`ambiguous`: the cutoff, rank deficiency, kappa >= ~1e5, inverted ties): such a particle is judged on s^,
  Jp', hf and |det F_E| = prod s^ only, and the share of such particles in a scene is capped at plastic_truth.AMBIGUOUS_MAX — a
  condition of the scene (`scene` draws the hazardous matrices rarely enough), asserted on the CPU from the truth alone.
- tau, through C' = grad m - tau V0 (4 / h^2) dt, by transfer_truth.Particles.affine as for every particle: tau in fp64 of the F the
  kernel stored, C_TAU u devmath_truth.tau_scales — linear in (lambda, mu), so handing it lambda hf, mu hf scales the bound by hf.
  hf there is the fp64 factor of the STORED Jp' (`hardened`): what a read-out recomputes. The kernel's own fp32 factor differs from it
  by the fp32 evaluation alone, relative C_DP u (|xi Jp'| + |e| + 1), added times coeff |tau|.
"""
import copy
from typing import NamedTuple

import numpy as np

import devmath_truth as DM
import plastic_truth as PT
import transfer_truth as T
from helpers import report_margin

U32 = T.U32
H_OF = PT.H_OF
JP_IN = (1.0, 0.6, 1.4, 0.0, 0.3)      # 0.3 and 0: xi (1 - Jp) = 7 and 10 > the cap of 5
THETA_C, THETA_S, XI, CAP = 2.5e-2, 7.5e-3, 10.0, 5.0
HAZARD_SHARE = 0.012                    # of a scene's particles drawn from the families whose direction is arbitrary: under the cap of 0.02

CASES = {
    # name: (uni_dp layout the library will pick, fracture, per-particle mass / material, WGS_DEBUG switch, collider)
    "layout2": (2, False, True, None, False),
    "layout1_switch_per_particle": (1, False, True, None, False),
    "layout0_parameters_per_particle": (0, False, True, None, False),
    "layout2_uniform_material": (2, False, False, None, False),          # 3D: mass and material are kernel arguments
    "layout1_collider": (1, False, True, None, True),                    # the pair kernel, list half
    "layout1_fracture": (1, True, True, None, False),
    "forced_layout0": (2, False, False, "NO_UNIFORM", False),
    "layout2_two_pass": (2, False, False, "G2P_TWO_PASSES", False),
    "layout1_collider_no_dense": (1, False, True, "NO_G2P_DENSE", True),
}
CASE_IDS = [(c, d) for c in sorted(CASES) for d in (2, 3) if not (c == "layout2_uniform_material" and d == 2)]
STEADY = [("layout2", 3, 0.5), ("layout1_switch_per_particle", 2, 0.5)]


# ------------------------------------------------------------------------------------------------ the rule
def box(dp):
    dp = np.asarray(dp, np.float64)
    return 1.0 - dp[:, 0], 1.0 + dp[:, 1]


def hardening64(dp, jp):
    dp = np.asarray(dp, np.float64)
    e = np.minimum(dp[:, 2] * (1.0 - np.asarray(jp, np.float64)), dp[:, 3])
    return np.exp(e), e


def project64(F, dp, jp, svd=None):
    """(F_E [n,d,d], Jp', s^ [n,d] in the SVD's order, (U, s, V)) of the rule on every row, gate or not"""
    F = np.asarray(F, np.float64)
    U, s, V = DM.svd_lapack(T.unmat(F)) if svd is None else svd
    lo, hi = box(dp)
    sh = np.clip(s, lo[:, None], hi[:, None])
    jp2 = np.asarray(jp, np.float64) * np.prod(np.abs(s), 1) / np.prod(sh, 1)
    return (U * sh[:, None, :]) @ np.transpose(V, (0, 2, 1)), jp2, sh, (U, s, V)


class Snow:
    """The truth of one substep's plastic block on trial matrices F [n, d, d] (exact fp32 values in float64), from the fp32 inputs
    dp [n, 6], state [n, 3], phase [n, 2] of the substep."""

    def __init__(self, F, dp, state, phase):
        F = np.asarray(F, np.float64)
        self.n, self.d = n, d = F.shape[0], F.shape[1]
        self.F = F
        self.dp32, self.state32 = np.asarray(dp, np.float32), np.asarray(state, np.float32)
        self.dp, self.state = self.dp32.astype(np.float64), self.state32.astype(np.float64)
        self.fr = fr = PT.Fracture(F, None, phase)
        self.has = self.dp[:, 4] != 0.0
        self.cand64 = (fr.phase64 == 0.0) & self.has
        self.F_E, self.jp, self.sh, self.svd = project64(F, self.dp, self.state[:, 0], fr.svd)
        U, s, V = self.svd
        self.hf, self.e = hardening64(self.dp, self.jp)
        a = np.abs(s)
        smax = np.maximum(a.max(1), 1e-300)
        sv = DM.C_SV * U32 * smax
        self.fn, self.fen = np.linalg.norm(F, axis=(1, 2)), np.linalg.norm(self.F_E, axis=(1, 2))
        self.b_sh = sv + DM.C_REC * U32 * self.fen
        others = np.stack([np.prod(np.delete(a, k, 1), 1) for k in range(d)], 1)
        psh = np.prod(self.sh, 1)
        self.b_jp = DM.C_DP * U32 * np.abs(self.state[:, 0]) * ((smax[:, None] * others).sum(1) +
                                                                   np.prod(a, 1) * (d + 2.0 + (smax[:, None] / self.sh).sum(1))) / psh
        self.b_hf = self.hf * (np.abs(self.dp[:, 2]) * self.b_jp + DM.C_DP * U32 * (np.abs(self.e) + 1.0))
        ang = DM.C_VEC * U32 * smax[:, None] / np.maximum(a, 1e-300)                  # [n, d]
        order = np.argsort(a, 1)
        i0, i1 = order[:, 0], order[:, 1]
        r = np.arange(n)
        flip = s.min(1) < sv                                                          # inverted, or a sign the fp32 values cannot tell
        ang_flip = np.where(flip, DM.C_VEC * U32 * smax / np.maximum(a[r, i1] - a[r, i0], 1e-300), 0.0)
        self.ambiguous = (ang.max(1) >= DM.VEC_MAX_BOUND) | (ang_flip >= DM.VEC_MAX_BOUND)
        self.b_FE = DM.C_REC * U32 * (self.fn + self.fen) + (self.sh * ang).sum(1) + (self.sh[r, i0] + self.sh[r, i1]) * ang_flip
        self.clamped = np.any(self.sh != s, axis=1)

    def ambiguous_share(self, cand=None):
        cand = (self.cand64 | (self.fr.amb_frac & self.has)) if cand is None else cand
        return float((cand & self.ambiguous).sum()) / self.n


class Judged(NamedTuple):
    cand: np.ndarray        # [n] the judged run sent the particle through the projection (its own phase == 0, dp[4] != 0)
    ratio: dict             # quantity -> [n] error / bound (0 where not a candidate)
    bad: np.ndarray         # [n] any complaint
    amb: np.ndarray         # [n] candidates judged without their direction
    hf: np.ndarray          # [n] fp64 hardening factor of the STORED Jp (1 where not a candidate): what a read-out recomputes
    b_hf_rel: np.ndarray    # [n] relative distance of the kernel's own fp32 factor from it


def judge(tag, sn: Snow, got, fails, F_trial32=None):
    """Every particle's phase, def_grad and dp_state of a run (ParticleSet or dict) against the truth.
    - phase, and the state and F of a particle that did not pass the gate: plastic_truth.gate;
    - one that did: state words 1 and 2 bit for bit, Jp', s^ (the singular values of the stored F), |det F_E| and — unless its
      direction is arbitrary — F_E, each within its bound."""
    g = PT._get(got)
    d = sn.d
    F_out = T.mat(np.asarray(g("def_grad"), np.float64), d)
    st = np.asarray(g("dp_state"))
    cand, _, bad, complain = PT.gate(tag, sn.fr, sn.has, sn.state32, got, fails, F_trial32)
    complain(cand & ~np.all(st[:, 1:] == sn.state32[:, 1:], axis=1), "state word 1 or 2 (plastic_hardening, log_vol_gain) touched")
    ratio = {}

    def held(name, err, bound, sel):
        r = np.where(sel, err / np.maximum(bound, 1e-300), 0.0)
        r = np.where(sel & ~np.isfinite(err), np.inf, r)
        ratio[name] = r
        report_margin(f"{tag}: snow {name}, worst error / bound", float(r.max()) if sel.any() else 0.0, 1.0, n=int(sel.sum()), failures=int((r > 1.0).sum()))
        complain(r > 1.0, f"snow {name} over its bound (worst {float(r.max()):.3g} x)")

    sv_got = np.sort(np.linalg.svd(F_out, compute_uv=False), 1)
    held("clamped singular values", np.abs(sv_got - np.sort(sn.sh, 1)).max(1), sn.b_sh, cand)
    held("Jp'", np.abs(st[:, 0].astype(np.float64) - sn.jp), sn.b_jp, cand)
    complain(cand & ~(st[:, 0] >= 0.0) & (sn.state[:, 0] >= 0.0), "Jp' < 0")
    psh = np.prod(sn.sh, 1)
    held("|det F_E|", np.abs(np.abs(np.linalg.det(F_out)) - psh), d * psh * sn.b_sh / np.min(sn.sh, 1), cand)
    held("F_E", np.linalg.norm(F_out - sn.F_E, axis=(1, 2)), sn.b_FE, cand & ~sn.ambiguous)
    hf_stored, e_stored = hardening64(sn.dp, st[:, 0].astype(np.float64))
    held("hf of the stored Jp'", np.abs(hf_stored - sn.hf), sn.b_hf, cand)
    hf = np.where(cand, hf_stored, 1.0)
    rel = np.where(cand, DM.C_DP * U32 * (np.abs(sn.dp[:, 2] * st[:, 0]) + np.abs(e_stored) + 1.0), 0.0)
    return Judged(cand, ratio, bad, cand & sn.ambiguous, hf, rel)


def report_ambiguous(tag, jd: Judged, sn: Snow, fails):
    n = sn.n
    amb = jd.amb | sn.fr.amb_frac
    report_margin(f"{tag}: particles judged without their direction, or inside the fracture band (fraction)", float(amb.sum()) / n, PT.AMBIGUOUS_MAX,
                  count=int(amb.sum()))
    if not amb.sum() <= PT.AMBIGUOUS_MAX * n:
        fails.append(f"{tag}: {int(amb.sum())} of {n} particles are ambiguous (cap {PT.AMBIGUOUS_MAX})")


def hardened(pt, hf):
    """transfer_truth.Particles whose stress takes lambda hf, mu hf (check_particles then holds C' of a snow run)"""
    out = copy.copy(pt)
    out.inp = copy.copy(pt.inp)
    out.inp.lam, out.inp.mu = pt.inp.lam * hf, pt.inp.mu * hf
    return out


def check_particles(tag, pt, got, jd: Judged, fails, sel=None):
    """transfer_truth.check_particles with the hardened coefficients; F of the gate's particles is judge's. The kernel's own fp32 hf
    against the fp64 one of the stored Jp' enters C' as coeff |tau| b_hf_rel: checked here on its own, on top of affine's bound."""
    ph = hardened(pt, jd.hf)
    T.check_particles(tag, ph, got, 0, fails, sel=_without(sel, jd.cand))
    m = jd.cand if sel is None else jd.cand & np.asarray(sel, bool)
    if m.any():
        g = PT._get(got)
        # (x and v of the gate's particles: transfer_truth.check_particles' own two lines, its C' with the term above)
        T.check(f"{tag}: x of the snow particles", np.linalg.norm(np.asarray(g("pos"), np.float64) - pt.x, axis=1), pt.b_x, fails, m)
        T.check(f"{tag}: v of the snow particles", np.linalg.norm(np.asarray(g("vel"), np.float64) - pt.vel, axis=1), pt.b_vel, fails, m)
        Fg = np.asarray(g("def_grad"), np.float64)
        Cn, bC = ph.affine(0, Fg)
        tau = (pt.grad * pt.inp.m[:, None, None] - Cn) / np.maximum(pt.inp.vol * pt.invd * pt.dt, 1e-300)[:, None, None]
        extra = pt.inp.vol * pt.invd * pt.dt * np.linalg.norm(tau, axis=(1, 2)) * jd.b_hf_rel
        T.check(f"{tag}: C' of the snow particles (hardened stress)", np.linalg.norm(T.mat(np.asarray(g("affine"), np.float64), pt.d) - Cn, axis=(1, 2)),
                bC + extra, fails, m)


def _without(sel, mask):
    keep = ~np.asarray(mask, bool)
    return keep if sel is None else np.asarray(sel, bool) & keep


# ------------------------------------------------------------------------------------------------ scenes
def _near_box(rng, n, d):
    """every axis below, inside and above [1 - theta_c, 1 + theta_s], independently"""
    s = 1.0 + np.where(rng.random((n, d)) < 0.34, rng.uniform(-0.08, -THETA_C, (n, d)),
                       np.where(rng.random((n, d)) < 0.5, rng.uniform(-THETA_C, THETA_S, (n, d)), rng.uniform(THETA_S, 0.06, (n, d))))
    return T.unmat(DM._usv(rng, s)).astype(np.float32)


def draw_F(d, n, rng):
    """(F [n, d*d] fp32, family per row): every matrix of devmath_truth.catalogue whose direction the clamp can use, the hazardous
    ones (ambiguous under Snow's own criterion with the scene's default box) at HAZARD_SHARE of the scene, the rest near the box."""
    cat = DM.catalogue(d, seed=3)
    F = np.concatenate(list(cat.values()))
    fam = np.concatenate([[k] * len(v) for k, v in cat.items()])
    dp = np.tile(np.array([THETA_C, THETA_S, XI, CAP, 1.0, 0.0], np.float32), (len(F), 1))
    one = np.tile(np.array([1.0, 1.0, 0.0], np.float32), (len(F), 1))
    hazard = Snow(T.mat(F, d), dp, one, np.zeros((len(F), 2), np.float32)).ambiguous
    keep = np.nonzero(~hazard)[0]
    hz = rng.permutation(np.nonzero(hazard)[0])[: int(HAZARD_SHARE * n)]
    pick = np.concatenate([keep, hz])
    if len(pick) > n // 2:                                  # (2D at 1 500: the catalogue is a third of the scene)
        pick = np.concatenate([rng.permutation(keep)[: n // 2 - len(hz)], hz])
    nb = _near_box(rng, n - len(pick), d)
    F = np.concatenate([F[pick], nb])
    fam = np.concatenate([fam[pick], np.full(len(nb), "near_box")])
    p = rng.permutation(n)
    return F[p].copy(), fam[p]


def scene(case, d, h=None, seed=0, steady=False, n=None):
    """(scene dict with "plasticity", family per particle): plastic_truth.scene's block of particles in its velocity field, F from
    `draw_F` (steady: near I), Jp_in from JP_IN, state words 1 and 2 random. Layout 1: every third particle has the switch off (an
    elastic corotated particle under phase 0); layout 0: theta_c, theta_s and xi per particle. Fracture: every other particle breakable
    (phase 1) with max_stretch inside plastic_truth.STRETCH_WINDOW of s_max(F_in), F of those from the moderate families."""
    from wgsparkl_amd.models import PLASTICITY_SNOW, Snow as SnowParams
    layout, fracture, per_particle, _, collider = CASES[case]
    base_case = "mode1_fracture_collider" if collider else ("mode1_fracture_corotated" if per_particle else "mode2_fracture_uniform_material")
    sc, _ = PT.scene(base_case, d, h=h, seed=seed + 100, steady=steady, n=n, elastic=0.0)
    ps = sc["particles"]
    n = ps.n
    rng = np.random.default_rng(8100 + 31 * seed + 7 * d + sorted(CASES).index(case))
    if steady:
        s = np.exp(rng.normal(-0.01, 0.03, (n, d)))
        F, fam = T.unmat(DM._usv(rng, s)).astype(np.float32), np.full(n, "near_identity")
    else:
        F, fam = draw_F(d, n, rng)
    ps.dp[:] = SnowParams(THETA_C, THETA_S, XI, CAP).as_array()
    ps.has_plasticity[:] = True
    ps.has_phase[:] = True
    ps.phase[:] = np.array([0.0, -1.0], np.float32)
    if layout == 1:
        ps.dp[::3, 4] = 0.0
    if layout == 0:
        ps.dp[:, 0] = (THETA_C * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        ps.dp[:, 1] = (THETA_S * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        ps.dp[:, 2] = rng.uniform(5.0, 15.0, n).astype(np.float32)
    if fracture:
        cat = DM.catalogue(d, seed=5)
        mod = np.concatenate([v for k, v in cat.items() if k == "well_conditioned" or k.startswith("clustered")])
        br = np.zeros(n, bool)
        br[rng.permutation(n)[: n // 2]] = True
        F[br] = mod[rng.integers(0, len(mod), int(br.sum()))]
        fam[br] = "breakable"
        ms = (PT._s_max(F, d) * (1.0 + rng.uniform(*PT.STRETCH_WINDOW, n))).astype(np.float32)
        ps.phase[br, 0] = 1.0
        ps.phase[br, 1] = ms[br]
    ps.def_grad[:] = F
    jp = np.asarray(JP_IN, np.float32)[rng.integers(0, len(JP_IN), n)]
    if steady:
        jp = rng.uniform(0.8, 1.2, n).astype(np.float32)
    ps.dp_state[:] = np.stack([jp, rng.uniform(0.0, 2.0, n).astype(np.float32), rng.uniform(-0.2, 0.2, n).astype(np.float32)], 1)
    sc["plasticity"] = PLASTICITY_SNOW
    return sc, fam
