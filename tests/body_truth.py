"""fp64 truth of what the rigid bodies receive from the CPIC transfer and of how they integrate (oracle/mpm_oracle.c: the
impulse part of orc_p2g, flt2int, orc_integrate_bodies, orc_update_world_mass_properties), with rounding bounds. Built on
tests/cpic_truth.py: a cpic_truth.Result holds the (particle, node) pairs that do not transfer, their ghost velocities and
the bound of each.

The discrete decisions are inputs: cpic_truth's (which pairs are incompatible, each node's closest body), the poses and
velocities of the bodies before the substep (`State`), their mass properties (`Props`).

Two stages:
- `impulses`: per (node, body) the sum over the node's pairs of delta_impulse and cross(delta_impulse, com - cell_center),
  as an interval [lo, hi] per axis; per body the sum of flt2int of the two ends (truncation toward zero is monotone): an
  integer interval per body and axis. flt2int saturates at +-2^31 and the sum wraps modulo 2^32, as in the reference;
  `Impulses.in_range` says whether a case stays clear of both.
- `integrate`: the body update from an accumulator interval: the candidates (one per side of a cap the body is near to)
  of linvel, angvel, translation, rotation and com, each with a normwise bound.

Bounds are fixed multiples of u = 2^-24 times stated scales; the multiples were settled against the C fp32 oracle in
tests/test_body_truth.py (and hold for the C fp64 oracle with u = 2^-53), never against the kernels. The fixed-point
conversions are fp32 in every flavour (the fp64 oracle casts to float too): their roundings are multiples of U32 whatever u is.

Shared by tests/test_body_truth.py (CPU) and tests/test_gpu_bodies.py (the HIP kernels)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import cdf_truth as CT
import cpic_truth as CP
import transfer_truth as T
from helpers import report_margin

U32, U64 = T.U32, T.U64
UNITS = 1.0e5             # the fixed point: one unit is 1e-5 (exactly representable in fp32)
I31, I32 = 1 << 31, 1 << 32
NEAR_MAX = 0.1            # share of the checked bodies that may be near a cap (either side accepted)
SENSITIVE = 4.0           # a node counts as seen when its contribution moves a velocity by more than this many bounds
SHARE_MIN = 0.9

# ---- fixed multiples of u
# a pair's delta_impulse (v_p - ghost) (w m): the difference (1), w m (1), the product (1), and one spare for a fused / unfused form
C_DIMP = 4.0
# its angular part cross(dimp, lever): per component two products and a difference (3), sqrt(3) in the norm: 3 sqrt(3) ~ 5, the lever's own
# rounding (1): 6 of |dimp| |lever|; the lever com - cell_center also carries the absolute error of the cell centre (u dpt_error + u |cc|)
C_CROSS = 6.0
# the sum of a node's n pairs in any order: (n - 1) u of sum |term|, C_SUM more for the partial sums kept in other formats of the same
# precision (the per-wave tiles, the block sum, the gather over 2^D slabs: adding an exact 0 costs nothing, so these are not levels)
C_SUM = 2.0
C_FIX = 2.0       # (float) of the total and its product by 1e5, and back: (float) of the integer and its division by 1e5; of U32 always
# applyImpulse: inv_mass * lin (1) and the sum (1), twice for the norms' sake: 4 of |v| + |dv|
C_APPLY = 4.0
# the world inverse inertia R I R^T: R from the quaternion (~6 roundings an entry), two 3-term products (3 + 3), its product with ang (3),
# sqrt(3) for the norm: ~ 32 of |I_local| |ang|
C_INERTIA = 32.0
C_CAP = 8.0       # the cap v (lim / |v|): fl(0.1) (1), h (1), / dt (2), |v| (D + 1), the quotient (1), the product (1); of lim
# the world centre of mass pose * local_com where local_com itself came from an fp32 pose^-1 * com: each a rotation (3-term sums of
# products, ~8) of the scale |trans| + |arm|
C_POSE = 16.0
C_TRIG = 8.0      # sin, cos of the device (a few ulp) and the rotation of the arm (3-term sums): of |arm|
C_ROT = 16.0      # the Hamilton product (4-term sums of products: 8), the norm and the division (4), sin / cos (4): absolute, |q| = 1
C_SUMS = 4.0      # a sum of three terms and a product by dt: of the terms' magnitudes

VARIANTS = ("lever_from_translation", "angular_sign", "body_lowest_bit", "round_to_nearest", "truncate_per_body", "truncate_per_pair",
            "caps_without_impulse", "no_caps", "linear_cap_h_dt", "gravity_before_pose", "gravity_on_kinematic_axes",
            "rotate_about_translation", "local_inertia")


# ------------------------------------------------------------------------------------------------ inputs
class Props:
    """inv_mass [nb, d], inv_inertia_local [nb] (2D) or [nb, 3, 3] (3D, from the column-major 9), scale [nb] of the scene's first 16 colliders"""

    def __init__(self, colliders, d):
        cols = list(colliders)[:16]
        self.d, self.n = d, len(cols)
        self.inv_mass = CT.f32(np.array([(list(c.inv_mass) + [0.0] * 3)[:d] for c in cols], np.float64).reshape(-1, d))
        ii = CT.f32(np.array([(list(c.inv_inertia_local) + [0.0] * 9)[:9] for c in cols], np.float64).reshape(-1, 9))
        self.inv_inertia = ii[:, 0].copy() if d == 2 else ii.reshape(-1, 3, 3).transpose(0, 2, 1).copy()
        self.scale = np.array([float(c.scale) for c in cols], np.float64)


class State(NamedTuple):
    """read_body_poses() / collider_states() of one body: rotation (2D: cos, sin; 3D: the quaternion i, j, k, w), translation, linvel, angvel, com"""
    rotation: np.ndarray
    translation: np.ndarray
    linvel: np.ndarray
    angvel: np.ndarray
    com: np.ndarray

    @staticmethod
    def of(pose):
        return State(*(np.asarray(pose[k], np.float64) for k in State._fields))


def rot_matrix(rot, d):
    if d == 2:
        c, s = rot
        return np.array([[c, -s], [s, c]])
    x, y, z, w = rot
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ------------------------------------------------------------------------------------------------ what the bodies receive
def flt2int(x, variant=()):
    """i32(x * 1e5) of fp64 x: toward zero, saturating at +-2^31, NaN -> 0; as Python-sized integers (int64)"""
    s = np.asarray(x, np.float64) * UNITS
    s = np.where(np.isnan(s), 0.0, s)
    t = np.rint(s) if "round_to_nearest" in variant else np.trunc(s)
    return np.clip(t, -float(I31), float(I31 - 1)).astype(np.int64)


def wrap(a):
    """an int64 sum as the int32 accumulator holds it"""
    return ((np.asarray(a, np.int64) + I31) % I32) - I31


class Impulses:
    """lo, hi [nb, d + na] int64: the unwrapped sums of flt2int of the interval ends; the (node, body[, rank]) totals behind them"""

    def __init__(self, lo, hi, body, tot, bound, saturating, d, exchanges=None):
        self.lo, self.hi, self.d = lo, hi, d
        self.exchanges = np.ones(len(body), bool) if exchanges is None else exchanges   # groups with a pair whose ghost velocity is not the particle's own (project_velocity's branch is not `away`)
        self.body, self.tot, self.bound = body, tot, bound       # per (node, body, rank) group: the body, the total [G, d + na], its bound [G, 2] (linear, angular)
        self.saturating = saturating                             # groups within their bound of +-2^31 units

    @property
    def in_range(self):
        """no node within its bound of saturation and every |sum| < 2^30: neither flt2int's saturation nor the wrap is in play"""
        return not self.saturating.any() and bool((np.abs(self.lo) < (1 << 30)).all() and (np.abs(self.hi) < (1 << 30)).all())

    def contains(self, acc):
        """[nb, d + na] bool: the int32 accumulators lie in the (wrapped) interval"""
        acc = np.asarray(acc, np.int64).reshape(self.lo.shape)
        width = self.hi - self.lo
        return ((acc - self.lo) % I32 <= width) | (width >= I32)

    def nodes(self, b):
        """number of (node, rank) groups that give body b a non-zero total"""
        return int(((self.body == b) & (np.abs(self.tot).sum(1) > 0)).sum())


def impulses(res: CP.Result, inp: T.Inputs, motion: CP.Motion, u=U32, variant=(), held=None, nb=None):
    """The accumulators of every body from a cpic_truth.Result (its pairs with nclosest < motion.n). `held` [n]: the rank that
    holds each particle (slabs truncate per (node, rank) and add the integers); None: one domain."""
    d, st, gr = inp.d, res.st, res.grid
    na = 1 if d == 2 else 3
    nb = motion.n if nb is None else nb
    p, s, ghost, bg = gr.pairs
    M = len(gr.keys)
    wm = st.w[p, s] * inp.m[p]
    dv = inp.v[p] - ghost
    dimp = dv * wm[:, None]
    cc = inp.x[p] + st.dpt[p, s]                              # the node position the pair used
    body = res.nclosest[p, s].astype(np.int64)
    if "body_lowest_bit" in variant:
        paff = res.contact.paff[p]
        low = np.zeros(len(p), np.int64)
        for c in range(15, -1, -1):
            low = np.where(((paff >> np.uint32(c)) & 1).astype(bool), c, low)
        body = np.minimum(low, nb - 1)
    com = (motion.trans if "lever_from_translation" in variant else motion.com)[body]
    lever = com - cc
    if d == 2:
        ang = (dimp[:, 0] * lever[:, 1] - dimp[:, 1] * lever[:, 0])[:, None]
    else:
        ang = np.cross(dimp, lever)
    if "angular_sign" in variant:
        ang = -ang
    term = np.concatenate([dimp, ang], 1)
    if "truncate_per_pair" in variant:
        term = flt2int(term).astype(np.float64) / UNITS
    nrm = lambda a: np.linalg.norm(a, axis=1)
    dn, ln = nrm(dimp), nrm(lever)
    # a pair: the ghost velocity's bound times w m, the weight's own error, the roundings of the difference and the products
    b_l = wm * bg + T.C_WT * u * st.weight_error[p] * inp.m[p] * nrm(dv) + C_DIMP * u * dn
    e_lever = u * (nrm(com) + 2.0 * nrm(cc) + st.dpt_error[p])
    b_a = b_l * ln + dn * e_lever + C_CROSS * u * dn * ln
    rank = np.zeros(len(p), np.int64) if held is None else np.asarray(held, np.int64)[p]
    key = (rank * nb + body) * M + gr.inv[p, s]
    gk, gi = np.unique(key, return_inverse=True)
    G = len(gk)
    gbody = (gk // M) % nb
    cnt = np.bincount(gi, None, G)
    tot = np.stack([np.bincount(gi, term[:, k], G) for k in range(d + na)], 1) if G else np.zeros((0, d + na))
    lvl = u * (cnt + C_SUM)
    B_l = np.bincount(gi, b_l, G) + lvl * np.bincount(gi, dn, G) + C_FIX * U32 * nrm(tot[:, :d])
    B_a = np.bincount(gi, b_a, G) + lvl * np.bincount(gi, dn * ln, G) + C_FIX * U32 * nrm(tot[:, d:])
    B = np.concatenate([np.repeat(B_l[:, None], d, 1), np.repeat(B_a[:, None], na, 1)], 1)
    sat = (np.abs(tot) + B).max(1) * UNITS >= float(I31) if G else np.zeros(0, bool)
    lo, hi = np.zeros((nb, d + na), np.int64), np.zeros((nb, d + na), np.int64)
    for b in range(nb):
        sel = gbody == b
        if "truncate_per_body" in variant:
            lo[b], hi[b] = flt2int((tot[sel] - B[sel]).sum(0), variant), flt2int((tot[sel] + B[sel]).sum(0), variant)
        else:
            lo[b], hi[b] = flt2int(tot[sel] - B[sel], variant).sum(0), flt2int(tot[sel] + B[sel], variant).sum(0)
    exch = np.bincount(gi, (res.ghost_branch[p, s] != 0).astype(np.float64), G) > 0 if G else np.zeros(0, bool)
    return Impulses(lo, hi, gbody, tot, np.stack([B_l, B_a], 1), sat, d, exch)


# ------------------------------------------------------------------------------------------------ how they integrate
class Outcome(NamedTuple):
    """one candidate of a body's state after the substep, with normwise bounds; `capped`: (linear, angular)"""
    value: State
    bound: State
    capped: tuple


class Body(NamedTuple):
    outcomes: list                 # one, or one per side of each cap the body is near to
    near: bool                     # more than one outcome is accepted
    impulse: bool                  # some accumulator is certainly non-zero
    speed: tuple                   # uncapped (|linvel|, |angvel|) after the impulse
    limits: tuple                  # (linear, angular) cap
    b_linvel: float                # the bounds of the uncapped velocities (the scale of `sensitivity`)
    b_angvel: float
    inertia_world: np.ndarray      # [na, na]


def _expm_apply(w_dt, q, arm, d):
    """(the rotation exp(w dt) composed with q, exp(w dt) applied to arm)"""
    if d == 2:
        a = float(w_dt[0])
        c, s = np.cos(a), np.sin(a)
        nq = np.array([c * q[0] - s * q[1], s * q[0] + c * q[1]])
        return nq / np.linalg.norm(nq), np.array([c * arm[0] - s * arm[1], s * arm[0] + c * arm[1]])
    angle = np.linalg.norm(w_dt)
    dq = np.array([0.0, 0.0, 0.0, 1.0])
    if angle != 0.0:
        dq = np.append(w_dt * (np.sin(0.5 * angle) / angle), np.cos(0.5 * angle))
    x, y, z, w = q
    nq = np.array([dq[3] * x + dq[0] * w + dq[1] * z - dq[2] * y, dq[3] * y - dq[0] * z + dq[1] * w + dq[2] * x,
                   dq[3] * z + dq[0] * y - dq[1] * x + dq[2] * w, dq[3] * w - dq[0] * x - dq[1] * y - dq[2] * z])
    return nq / np.linalg.norm(nq), rot_matrix(dq, 3) @ arm


def integrate(state: State, inv_mass, inv_inertia, lo, hi, h, dt, gravity, u=U32, variant=()):
    """One body through one substep from the interval [lo, hi] (int64, d + na) of its accumulators (wrapped by the caller
    where the case is out of range). inv_inertia: the local one (2D: a number; 3D: [3, 3])."""
    d = len(state.translation)
    na = 1 if d == 2 else 3
    nrm = np.linalg.norm
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid, hw = 0.5 * (lo + hi) / UNITS, 0.5 * (hi - lo) / UNITS
    lin, ang, hw_l, hw_a = mid[:d], mid[d:], hw[:d], hw[d:]
    inv_mass = np.asarray(inv_mass, np.float64)
    g = np.asarray(gravity, np.float64)[:d]
    # (the fp32 flavours hold h and dt as fp32; the fp64 oracle, checked with u = U64, as given)
    h32, dt32 = (float(np.float32(h)), float(np.float32(dt))) if u > 1.0e-10 else (float(h), float(dt))
    if d == 2:
        Iw = np.array([[float(inv_inertia)]])
        e_I = 0.0
    else:
        R = rot_matrix(state.rotation, 3)
        Il = np.asarray(inv_inertia, np.float64)
        Iw = Il if "local_inertia" in variant else R @ Il @ R.T
        e_I = C_INERTIA * u * nrm(Il)
    dvl, dva = inv_mass * lin, Iw @ ang
    nl, na_ = state.linvel + dvl, state.angvel + dva
    b_nl = nrm(inv_mass * hw_l) + C_APPLY * u * (nrm(state.linvel) + nrm(dvl)) + C_FIX * U32 * nrm(dvl)
    b_na = nrm(Iw, 2) * nrm(hw_a) + e_I * nrm(ang) + C_APPLY * u * (nrm(state.angvel) + nrm(dva)) + C_FIX * U32 * nrm(dva)
    certain = bool(((lo > 0) | (hi < 0)).any())
    maybe = bool(((lo != 0) | (hi != 0)).any())
    lim_l = (1.0 if "linear_cap_h_dt" in variant else 0.1) * h32 / dt32
    lim_a = 1.0
    sl, sa = nrm(nl), nrm(na_)

    def sides(speed, lim, b):
        """the cap decisions to accept: [False], [True] or both"""
        if "no_caps" in variant:
            return [False]
        with_imp = [speed > lim] if abs(speed - lim) > b + C_CAP * u * lim else [False, True]
        if "caps_without_impulse" in variant or certain:
            return with_imp
        return sorted(set(with_imp + [False])) if maybe else [False]

    outcomes = []
    for cap_l in sides(sl, lim_l, b_nl):
        for cap_a in sides(sa, lim_a, b_na):
            v = nl * (lim_l / sl) if cap_l else nl
            w = na_ * (lim_a / sa) if cap_a else na_
            # the cap x -> lim x / |x| contracts by lim / R among points of norm >= R >= lim: an error b of a speed sl shrinks by lim / (sl - b)
            b_v = b_nl * (lim_l / max(sl - b_nl, lim_l)) + C_CAP * u * lim_l if cap_l else b_nl
            b_w = b_na * (lim_a / max(sa - b_na, lim_a)) + C_CAP * u * lim_a if cap_a else b_na
            if "gravity_before_pose" in variant:
                v = v + np.where(inv_mass != 0.0, g * dt32, 0.0)
            comw = state.com
            arm = np.zeros(d) if "rotate_about_translation" in variant else state.translation - comw
            pivot = state.translation if "rotate_about_translation" in variant else comw
            an, tn = nrm(state.translation - comw), nrm(state.translation)
            # (a quaternion of fp32 entries is a unit one to U32 only, and rotating with it scales by |q|^2; the integration normalises it)
            e_com = C_POSE * u * (tn + an) + 2.0 * abs(float(np.dot(state.rotation, state.rotation)) - 1.0) * an
            q, rarm = _expm_apply(w * dt32, state.rotation, arm, d)
            trans = pivot + rarm + v * dt32
            b_tr = 2.0 * e_com + an * (b_w * dt32 + C_TRIG * u) + dt32 * b_v + C_SUMS * u * (nrm(comw) + an + nrm(v) * dt32)
            b_q = (1.0 if d == 2 else 0.5) * b_w * dt32 + C_ROT * u
            dyn = np.ones(d, bool) if "gravity_on_kinematic_axes" in variant else inv_mass != 0.0
            vg = v if "gravity_before_pose" in variant else v + np.where(dyn, g * dt32, 0.0)
            b_vg = b_v + C_SUMS * u * (nrm(g) * dt32 + nrm(vg))
            # the refreshed world centre of mass pose' * local_com: the rotation about it leaves it where it was, the translation moves it
            if "rotate_about_translation" in variant:
                com = trans + _expm_apply(w * dt32, state.rotation, comw - state.translation, d)[1]
            else:
                com = comw + v * dt32
            b_com = b_tr + 4.0 * b_q * an + e_com
            outcomes.append(Outcome(State(q, trans, vg, w, com), State(b_q, b_tr, b_vg, b_w, b_com), (cap_l, cap_a)))
    return Body(outcomes, len(outcomes) > 1, certain, (sl, sa), (lim_l, lim_a), b_nl, b_na, Iw)


def ratios(out: Outcome, got: State):
    """error / bound of the five quantities (the quaternion up to sign)"""
    r = {}
    for k in State._fields:
        a, b = np.asarray(getattr(got, k), np.float64), getattr(out.value, k)
        e = np.linalg.norm(a - b)
        if k == "rotation" and len(b) == 4:
            e = min(e, np.linalg.norm(a + b))
        bound = float(getattr(out.bound, k))
        r[k] = (e, bound)
    return r


def sensitivity(imp: Impulses, b, body: Body, inv_mass, by_impulse=False):
    """per axis (d linear, na angular; NaN where the axis takes nothing): the share of the nodes contributing to body b whose
    own contribution, carried to the velocity, exceeds SENSITIVE times the velocity bound. A node contributes when one of its
    pairs exchanges momentum (a pair on project_velocity's `away` branch keeps the particle's own velocity: its delta_impulse
    is 0 by rule, and 1e-16 of rounding in this truth). `by_impulse`: the share of the units instead of the share of the
    nodes (what part of the accumulator comes from nodes that a velocity check would each see)."""
    d = imp.d
    tot = np.abs(imp.tot[(imp.body == b) & imp.exchanges])
    na = tot.shape[1] - d
    out = np.full(d + na, np.nan)
    inv_mass = np.asarray(inv_mass, np.float64)
    for k in range(d + na):
        gain = inv_mass[k] if k < d else np.linalg.norm(body.inertia_world[:, k - d])
        c = tot[:, k]
        if gain != 0.0 and len(c) and c.sum() > 0.0:
            seen = gain * c > SENSITIVE * (body.b_linvel if k < d else body.b_angvel)
            out[k] = float(c[seen].sum() / c.sum()) if by_impulse else float(seen.mean())
    return out


# ------------------------------------------------------------------------------------------------ checks
class BodyCheck(NamedTuple):
    bodies: list                   # the Body of every collider
    near: int                      # bodies near a cap
    fits: list                     # per body: the index of the outcome its state fits (-1: none)
    shares: np.ndarray             # [nb, d + na] sensitivity
    by_impulse: np.ndarray         # [nb, d + na] ... by units instead of by nodes


def check_accumulators(tag, imp: Impulses, acc, fails):
    """the int32 accumulators of every body inside the truth's interval (margin: the distance from the interval's middle over its half width)"""
    acc = np.asarray(acc, np.int64).reshape(-1)[:imp.lo.size].reshape(imp.lo.shape)
    ok = imp.contains(acc)
    half = 0.5 * (imp.hi - imp.lo).astype(np.float64)
    off = np.abs(wrap(acc - imp.lo).astype(np.float64) - half)
    i = int(np.argmax(off - half))
    report_margin(f"{tag}: accumulators (distance from the interval's middle, units of 1e-5)", float(off.reshape(-1)[i]), float(half.reshape(-1)[i]), n=int(acc.size))
    if not ok.all():
        b, k = np.argwhere(~ok)[0]
        fails.append(f"{tag}: {int((~ok).sum())}/{acc.size} accumulators outside the interval (first body {b} axis {k}: {acc[b, k]} not in [{imp.lo[b, k]}, {imp.hi[b, k]}])")


def check_bodies(tag, imp: Impulses, props: Props, before, after, h, dt, gravity, fails, u=U32, variant=(), scale=1.0, acc=None):
    """every body's state `after` the substep (a list of pose dicts) against the truth from the state `before` and the interval of
    its accumulators (or, `acc` given: from those accumulators exactly). `scale`: the bounds' multiple (the substep count of a
    free body's run)."""
    d = imp.d
    bodies, fits, near = [], [], 0
    worst = {k: (0.0, 1.0) for k in State._fields}
    # (out of range: the wrapped ends; a body whose interval straddles the wrap has lo > hi and is the caller's to exclude)
    lo, hi = (wrap(imp.lo), wrap(imp.hi)) if acc is None else (np.asarray(acc, np.int64).reshape(imp.lo.shape),) * 2
    for b in range(props.n):
        l, hh = lo[b], hi[b]
        assert (l <= hh).all(), f"{tag}: the accumulator interval of body {b} straddles the int32 wrap"
        body = integrate(State.of(before[b]), props.inv_mass[b], props.inv_inertia[b], l, hh, h, dt, gravity, u, variant)
        got = State.of(after[b])
        fit = -1
        for j, out in enumerate(body.outcomes):
            r = ratios(out, got)
            if all(e <= scale * bd for e, bd in r.values()):
                fit = j
                break
        r = ratios(body.outcomes[max(fit, 0)], got)
        for k, (e, bd) in r.items():
            if e * worst[k][1] >= worst[k][0] * scale * bd:
                worst[k] = (e, scale * bd)
        if fit < 0:
            bad = {k: f"{e:.3e} > {scale * bd:.3e}" for k, (e, bd) in r.items() if not e <= scale * bd}
            fails.append(f"{tag}: body {b} fits none of its {len(body.outcomes)} outcomes ({bad})")
        near += body.near
        bodies.append(body)
        fits.append(fit)
    for k, (e, bd) in worst.items():
        report_margin(f"{tag}: body {k}", e, bd, n=props.n)
    shares = np.array([sensitivity(imp, b, bodies[b], props.inv_mass[b]) for b in range(props.n)]) if props.n else np.zeros((0, 0))
    byi = np.array([sensitivity(imp, b, bodies[b], props.inv_mass[b], True) for b in range(props.n)]) if props.n else np.zeros((0, 0))
    return BodyCheck(bodies, near, fits, shares, byi)


def below_caps(body: Body):
    """the body took an impulse and its uncapped speeds lie clear below both caps"""
    return body.impulse and not body.near and not any(body.outcomes[0].capped)


def assert_sensitive(tag, ck: BodyCheck):
    """the share of every axis of every below-cap body is at least SHARE_MIN (a kinematic body takes nothing: no axis to see);
    returns the bodies it held for"""
    held = []
    for b, body in enumerate(ck.bodies):
        sh = ck.shares[b][~np.isnan(ck.shares[b])] if len(ck.shares) else np.zeros(0)
        if below_caps(body) and len(sh):
            report_margin(f"{tag}: nodes whose contribution a velocity check would see (share, lowest axis)", float(sh.min()), SHARE_MIN, body=b,
                          by_units=float(np.nanmin(ck.by_impulse[b])))
            assert sh.min() >= SHARE_MIN, (tag, b, ck.shares[b])
            held.append(b)
    return held


# ------------------------------------------------------------------------------------------------ scenes
def pow2(x):
    """the power of two nearest to x > 0 (in the exponent): an inv_mass whose product with an impulse is exact"""
    return float(2.0 ** np.rint(np.log2(x)))


MASS = 2048.0         # a dynamic body's mass in units of h^D: the impulses of a scene's particles (~h^(D+1) / dt) move it by a fifth of the linear cap
INERTIA = 2.0 ** 18   # ... and its inertia in units of h^(D+2): they turn it by less than 0.3 rad / s
LIGHT = 4096.0        # how much lighter a body meant to reach the linear cap is
LIGHT_INERTIA = 2.0 ** 16


def dynamic(col, d, h, locked=None, light_mass=1.0, light_inertia=1.0):
    """`col` as a dynamic body of mass MASS h^D (inv_mass a power of two: its product with an impulse is exact) and an inverse
    inertia of 1 / (INERTIA h^(D+2)); in 3D a diagonal of three different entries, so that world and local inertia differ
    under a rotation. `light_*` divide the mass / the inertia (a body meant to reach a cap); `locked`: an axis whose
    inv_mass is 0. Its angular velocity is halved (cpic_truth.moving's is 0.8 of the cap)."""
    import dataclasses
    inv_mass = [pow2(light_mass / (MASS * h ** d))] * 3
    if locked is not None:
        inv_mass[locked] = 0.0
    ii = pow2(light_inertia / (INERTIA * h ** (d + 2)))
    inertia = [ii] + [0.0] * 8 if d == 2 else [ii, 0, 0, 0, 0.5 * ii, 0, 0, 0, 2.0 * ii]
    ang = tuple(float(v) for v in CT.f32(0.5 * np.asarray(col.angvel, np.float64)))
    return dataclasses.replace(col, angvel=ang, inv_mass=tuple(inv_mass), inv_inertia_local=tuple(float(v) for v in inertia))


def faster(col, d, h, factor=3.0):
    """a kinematic body at `factor` times the linear cap and 2.5 rad / s"""
    import dataclasses
    lin = np.zeros(3)
    lin[:d] = (np.array([0.6, -0.64, 0.48]) * (factor * 0.1 * h / T.DT))[:d]
    if d == 2:
        lin[:2] = np.array([0.6, -0.8]) * (factor * 0.1 * h / T.DT)
    ang = (2.5,) if d == 2 else (1.5, -1.2, 1.6)
    f = lambda a: tuple(float(v) for v in CT.f32(a))
    return dataclasses.replace(col, linvel=f(lin), angvel=f(ang), inv_mass=(0.0,) * 3, inv_inertia_local=(0.0,) * 9)


# per scene: what each body is, and what the case is named after (checked by `reached`)
ROLES = dict(
    cuboid=("linear_cap",),                                # a rotated cuboid of unequal half extents, the centre of mass off the translation
    capsule=("angular_cap",),
    two_equal=("linear_cap", "angular_cap", "fast_touched"),
    ball=("angular_cap", "linear_cap", "fast_untouched"),  # (no particle reaches the ball at the origin)
    sixteen=("linear_cap", "kinematic") * 8,
)
# These five scenes hold no dynamic body below the caps: with 30 to 300 contributing nodes per body they cannot meet the sensitivity
# condition (see `sensitivity` and notes/round_24.md). Bodies below the caps are the business of `lone` and its kin below.


DRIFT = (-0.5, 0.6, -0.3)     # the particles' common velocity in units of 0.1 h / dt
NOISE = 0.2                   # ... and the deviation of each from it, as a share of |DRIFT|


def scene(name, d, h, model=0, uniform=False):
    """cpic_truth.SCENES[name] with its bodies given the mass properties and velocities of ROLES[name]; dynamic bodies move at
    half of cpic_truth.moving's speed (ulp(v) small against the 1e-5 quantum). The particles move together (DRIFT, NOISE): with
    cpic_truth's independent velocities a node's ~100 pairs cancel to a tenth of their sum while their bounds add up, and no
    single node's contribution stands out of the sum of all nodes' bounds (measured: a share of 0.1 in 3D); moving together
    the pairs of a node add up like their bounds do."""
    sc = CP.SCENES[name](d, h, model=model, uniform=uniform)
    ps = sc["particles"]
    rng = np.random.default_rng(7000 + 10 * d + int(10 * h))
    s = 0.1 * h / T.DT
    drift = np.asarray(DRIFT)[:d] * s
    ps.vel[:] = (drift + rng.normal(0.0, NOISE * np.linalg.norm(drift), (ps.n, d))).astype(np.float32)
    base = dict(CP._STATIC[name](d, h, uniform=uniform))["colliders"][:16]
    cols = []
    for i, (c, role) in enumerate(zip(base, ROLES[name])):
        c = CP.moving(c, i, d, h, speed=0.5 if role != "kinematic" else 1.0)
        if role in ("below", "locked_y"):
            c = dynamic(c, d, h, locked=1 if role == "locked_y" else None)
        elif role == "linear_cap":
            c = dynamic(c, d, h, light_mass=LIGHT)
        elif role == "angular_cap":
            c = dynamic(c, d, h, light_inertia=LIGHT_INERTIA)
        elif role.startswith("fast"):
            c = faster(c, d, h)
        cols.append(c)
    sc["colliders"] = cols
    sc["roles"] = ROLES[name]
    return sc


def reached(tag, sc, imp: Impulses, ck: BodyCheck, before, after):
    """the case reached what its bodies are named after; returns the bodies whose sensitivity is asserted (the below-cap ones)"""
    below = []
    for b, role in enumerate(sc["roles"]):
        body = ck.bodies[b]
        out = body.outcomes[max(ck.fits[b], 0)]
        s0, s1 = State.of(before[b]), State.of(after[b])
        if role in ("below", "locked_y", "light"):
            assert imp.nodes(b) >= 1 and body.impulse, (tag, b, role, "no impulse")
            assert body.near or out.capped == (False, False), (tag, b, role, body.speed, body.limits)
            if not body.near and role != "light":
                below.append(b)
            if role == "locked_y":
                assert s1.linvel[1] == s0.linvel[1], (tag, b, "the locked axis changed its velocity")
        elif role == "linear_cap":
            assert body.impulse and body.speed[0] > body.limits[0] and out.capped[0], (tag, b, role, body.speed, body.limits)
        elif role == "angular_cap":
            assert body.impulse and body.speed[1] > body.limits[1] and out.capped[1], (tag, b, role, body.speed, body.limits)
        elif role == "fast_touched":
            assert body.impulse and out.capped == (True, True), (tag, b, role)
            # the cap times its own direction, to a few ulps, whatever the impulse
            for v0, v1, lim in ((s0.linvel, s1.linvel, body.limits[0]), (s0.angvel, s1.angvel, body.limits[1])):
                assert np.linalg.norm(v1 - v0 * (lim / np.linalg.norm(v0))) <= C_CAP * U32 * lim, (tag, b, role, v0, v1)
        elif role == "fast_untouched":
            assert imp.nodes(b) == 0 and not body.impulse, (tag, b, role)
            assert np.array_equal(s1.linvel, s0.linvel) and np.array_equal(s1.angvel, s0.angvel), (tag, b, "an untouched kinematic body changed its velocity")
    return below


class OracleBodies(NamedTuple):
    run: CP.OracleRun
    before: list                   # collider_states() before the substep (world mass properties updated)
    acc: np.ndarray                # impulses() after p2g [16, d + na]
    after: list                    # collider_states() after integrate_bodies and the next refresh


def oracle_substep(sc, dtype):
    """cpic_truth.oracle_substep with the bodies: the accumulators read after p2g, integrate_bodies at the end, and the world
    mass properties refreshed as the next substep would"""
    from helpers import oracle
    ps = sc["particles"]
    d = ps.dim
    st = oracle(d, dtype).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc.get("model", 0))
    st.update_world_mass_properties()
    before = st.collider_states()
    st.update_rigid_particles()
    st.sort_rigid()
    assert not st.overflow
    st.grid_update_cdf()
    st.p2g_cdf()
    st.g2p_cdf()
    st.g["impulses"][:] = 0
    st.p2g()
    acc = st.impulses().reshape(16, -1)
    st.grid_update()
    st.g2p()
    st.particle_update()
    cells, mv, _, aff, closest = st.grid_records()
    f = CP.Fields(st.arr["cdf_affinity"].copy(), st.arr["cdf_normal"].astype(np.float64), st.arr["cdf_dist"].astype(np.float64), cells, aff, closest)
    run = CP.OracleRun(f, cells, np.asarray(mv, np.float64), {k: v.copy() for k, v in st.arr.items()})
    st.integrate_bodies()
    st.update_world_mass_properties()
    return OracleBodies(run, before, acc, st.collider_states())


LONE_HEAVY = {2: 32.0, 3: 1024.0}                          # the lone particle's mass over that of the others: its node totals are ~1e5 units, not ~1e2
LONE_MASS, LONE_INERTIA = 128.0, 4096.0      # a hundred times the lone particle's mass, in units of h^D; its impulse at 1.5 h turns the body by ~0.05 rad / s


def lone(d, h, model=0, uniform=False, heavy=None, twin=False, shape="ball", locked=None, depth=0.6, off=0.02, word=0x1, push=-0.5):
    """The scene built to meet the sensitivity condition: a rotated dynamic ball near the origin (small cell indices: a small
    weight error) and ONE particle 0.6 h inside its surface, a hair off a node, moving into the body and carrying the previous
    sign that conflicts with the nodes inside the ball; sixty more particles far out of the ball's reach. Every node the
    particle is incompatible with gets one pair: the body's accumulators are the sum of at most 3^D node totals (6 in 2D,
    8 in 3D). `heavy`: the particle's mass over that of the others (default LONE_HEAVY: node totals of ~1e5 units; `quantum`
    below: of a few units, far above their bounds, so that the truncation itself is what is checked); `twin`: a second
    particle in the same cell (two pairs per node)."""
    heavy = LONE_HEAVY[d] if heavy is None else heavy
    import dataclasses
    from wgsparkl_amd.solver import Collider, SimulationParams
    rng = np.random.default_rng(90 + d)
    c0 = np.array([0.63, 0.41, 0.52]) * h
    r = float(np.float32(1.5 * h))
    n0 = np.array([0.6, 0.5, 0.62][:d])
    n0 /= np.linalg.norm(n0)
    x = (np.rint((c0[:d] + (r - depth * h) * n0) / h) + off) * h
    far = c0[:d] + np.array([9.0, 0.0, 0.0][:d]) * h + rng.uniform(-2.0, 2.0, (60, d)) * h
    pos = np.concatenate([x[None, :], far])
    if twin:
        pos[1] = x + np.array([0.05, -0.04, 0.03][:d]) * h
    body = Collider.ball(r, CT._v(c0, d), rotation=CT._rot(d)) if shape == "ball" else \
        Collider.cuboid(CT._v(np.array([1.5, 1.1, 1.3]) * h, d), CT._v(c0, d), rotation=CT._rot(d))
    col = CP.moving(body, 0, d, h, speed=0.5)
    col = dynamic(col, d, h)
    col = dataclasses.replace(col, inv_mass=tuple(0.0 if k == locked else pow2(1.0 / (LONE_MASS * LONE_HEAVY[d] * h ** d)) for k in range(3)),
                              inv_inertia_local=tuple(float(v) * INERTIA / (LONE_INERTIA * LONE_HEAVY[d]) for v in col.inv_inertia_local))
    mo = CP.Motion.of([col], d)
    s = 0.1 * h / T.DT
    vel = rng.normal(0.0, 0.2 * s, (len(pos), d))
    t = rng.normal(0.0, 1.0, d)
    t -= n0 * (t @ n0)
    vel[0] = mo.at(np.array([0]), x[None, :])[0][0] + (push * n0 + 0.3 * t / np.linalg.norm(t)) * s
    if twin:
        vel[1] = vel[0] * 0.8 + 0.05 * s
    sc = T._finish(pos, h, rng, vel=vel, uniform=uniform, model=model)
    ps = sc["particles"]
    ps.affine[:] = 0.0
    ps.def_grad[:] = np.eye(d, dtype=np.float32).reshape(-1)
    for k in ("mass", "init_volume"):
        getattr(ps, k)[:2 if twin else 1] *= np.float32(heavy)
    ps.cdf_affinity[:2 if twin else 1] = word
    sc.update(params=SimulationParams(gravity=T.GRAVITY[:d], dt=T.DT), colliders=[col], roles=("light",) if twin else (("below",) if locked is None else ("locked_y",)))
    sc["grid_capacity"] = max(sc["grid_capacity"], 256)
    return sc


QUANTUM_HEAVY = {2: 3.0 / 32.0}
# where the lone particle sits and what it carries, per dimension: the placements at which every node it exchanges momentum with
# weighs enough to be seen (found by a scan over depth, offset, sign and direction with the C fp32 oracle; 2D: 6 to 7 nodes, 3D: 2 to 4)
PLACE = {2: dict(depth=-0.6, off=0.02, word=0x10001, push=0.5), 3: dict(depth=-0.3, off=-0.35, word=0x1, push=-0.5)}


def quantum(d, h, **kw):
    """`lone` with two light particles in one cell: node totals of tens to hundreds of units whose bounds are far below one unit"""
    return lone(d, h, heavy=QUANTUM_HEAVY[d], twin=True, **PLACE[d], **kw)


ROLES.update(lone=("below",), lone_cuboid=("below",), lone_locked=("locked_y",), quantum=("light",))
BUILD = dict({name: (lambda name: lambda d, h, **kw: scene(name, d, h, **kw))(name) for name in ("cuboid", "capsule", "two_equal", "ball", "sixteen")},
             lone=lambda d, h, **kw: lone(d, h, **PLACE[d], **kw),
             lone_cuboid=lambda d, h, **kw: lone(d, h, shape="cuboid", **PLACE[d], **kw),       # rotated, unequal half extents, unequal inertia
             lone_locked=lambda d, h, **kw: lone(d, h, locked=1, **PLACE[d], **kw),
             quantum=quantum)
HS = (0.2, 0.5)
# (quantum at 2D h = 0.2 only, where its intervals are 0 or 1 unit wide: in 3D the twin leaves one of its two to four nodes below the
# threshold on one angular axis, a share of 0.5 to 0.75, and at 2D h = 0.5 one of seven on x, 0.86: those cases cannot meet the condition)
CASES = [(name, d, h) for name in BUILD for d in (2, 3) for h in HS if name != "quantum" or (d, h) == (2, 0.2)]


def out_of_range(d):
    """cpic_truth's cuboid at h = 2.0 with the mass of density 50 (what tests/test_gpu_cpic.py::test_dynamic_body runs at h = 0.2)"""
    import dataclasses
    sc = CP.SCENES["cuboid"](d, 2.0)
    sc["colliders"] = [dataclasses.replace(c.with_density(50.0, d), linvel=c.linvel, angvel=c.angvel) for c in sc["colliders"]]
    sc["roles"] = ("out_of_range",)
    return sc


def free_bodies(d, h=0.5, particles=5):
    """sixteen bodies of random pose, velocity (below the caps: nothing caps them anyway) and mass properties, one of them a fixed
    rotated collider, one with a locked axis, two kinematic; `particles` particles 40 h away from all of them (0: none)"""
    import dataclasses
    from wgsparkl_amd.solver import Collider, SimulationParams
    rng = np.random.default_rng(500 + d)
    f = lambda a: tuple(float(v) for v in CT.f32(a))
    cols = []
    for i in range(16):
        c0 = np.array([3.0 * (i % 4), 3.0 * (i // 4), 1.0 + 0.5 * i]) * h + rng.uniform(-0.4, 0.4, 3) * h
        if d == 3:
            q = rng.normal(size=4)
            rot = f(q / np.linalg.norm(q))
        else:
            rot = (float(np.float32(rng.uniform(-3.0, 3.0))),)
        shape = Collider.ball(float(np.float32(0.6 * h)), CT._v(c0, d), rotation=rot) if i % 2 else \
            Collider.cuboid(CT._v(np.array([0.7, 0.4, 0.5]) * h, d), CT._v(c0, d), rotation=rot)
        if i == 5:                                            # the fixed rotated collider
            cols.append(shape)
            continue
        lin = np.zeros(3)
        lin[:d] = rng.uniform(-1.0, 1.0, d) * 0.05 * h / T.DT
        ang = rng.uniform(-0.5, 0.5, 1 if d == 2 else 3)
        com = np.zeros(3)
        com[:d] = np.asarray(shape.translation)[:d] + rng.uniform(-0.5, 0.5, d) * h
        c = dataclasses.replace(shape, linvel=f(lin), angvel=f(ang), com=f(com[:d]))
        if i not in (3, 9):                                   # (3 and 9: kinematic)
            m = rng.uniform(0.5, 4.0)
            ii = rng.uniform(0.5, 4.0, 3)
            c = dataclasses.replace(c, inv_mass=tuple(0.0 if (i == 7 and k == 0) else float(np.float32(1.0 / m)) for k in range(3)),
                                    inv_inertia_local=f([1.0 / ii[0]] + [0.0] * 8) if d == 2 else f([1.0 / ii[0], 0, 0, 0, 1.0 / ii[1], 0, 0, 0, 1.0 / ii[2]]))
        cols.append(c)
    pos = (np.array([60.0, 60.0, 60.0][:d]) + rng.uniform(-1.0, 1.0, (particles, d))) * h
    if particles:
        sc = T._finish(pos, h, rng, vel=np.zeros((particles, d)))
    else:
        from wgsparkl_amd.models import ElasticCoefficients, ParticlePhase
        from wgsparkl_amd.solver import ParticleSet
        ps = ParticleSet.uniform(pos.astype(np.float32), h / 4.0, 10.0, ElasticCoefficients.from_young_modulus(1e5, 0.3), phase=ParticlePhase(1.0, -1.0))
        sc = dict(particles=ps, cell_width=float(h), model=0, grid_capacity=256)
    sc.update(params=SimulationParams(gravity=T.GRAVITY[:d], dt=T.DT), colliders=cols, fixed=5)
    sc["grid_capacity"] = max(sc["grid_capacity"], 256)
    return sc


def check_free(tag, sc, before, after, count, fails):
    """`count` substeps of bodies that receive nothing: the truth iterated from `before`, the bound `count` times the last substep's"""
    d, h = sc["particles"].dim, sc["cell_width"]
    props = Props(sc["colliders"], d)
    worst = {k: (0.0, 1.0) for k in State._fields}
    zero = np.zeros(d + (1 if d == 2 else 3), np.int64)
    for b in range(props.n):
        state = State.of(before[b])
        for _ in range(count):
            body = integrate(state, props.inv_mass[b], props.inv_inertia[b], zero, zero, h, sc["params"].dt, sc["params"].gravity)
            assert len(body.outcomes) == 1 and body.outcomes[0].capped == (False, False)
            state = body.outcomes[0].value
        r = ratios(body.outcomes[0], State.of(after[b]))
        for k, (e, bd) in r.items():
            if e * worst[k][1] >= worst[k][0] * count * bd:
                worst[k] = (e, count * bd)
            if not e <= count * bd:
                fails.append(f"{tag}: body {b} {k}: {e:.3e} > {count} x {bd:.3e}")
    for k, (e, bd) in worst.items():
        report_margin(f"{tag}: body {k}", e, bd, n=props.n)
