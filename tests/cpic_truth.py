"""fp64 truth of the CPIC transfer: what P2G, G2P and the particle update do with the collider distance fields once they
exist (oracle/mpm_oracle.c: affinities_are_compatible, project_velocity, velocity_at_point, the node_mv part of orc_p2g,
orc_g2p, orc_particle_update), with per-element rounding bounds. Built on tests/transfer_truth.py: the stencil, the gated
node sums (Grid(gate=...)) and the G2P / update of given node velocities (Particles(contact=...)) are its classes.

The discrete decisions are inputs (`Fields`): per particle the affinity word, cdf_normal and cdf_dist of this substep, per
node the affinity word and the closest collider, per collider linvel, angvel and com before the substep (`Motion`). They
are checked by tests/cdf_truth.py and carry undecided sets of their own; a wrong decision there only moves elements
between the branches here. What this truth decides itself is sd < -0.05 h and max(sd, -0.3 h): particles whose sd lies
within C_THR u h of either are `near` (either side accepted for the first, which is a jump; the second is continuous and
its bound carries the difference), counted together with the particles near the speed cap.

Shared by tests/test_cpic_truth.py (CPU: the truth against the C fp64 oracle, the bounds against the C fp32 oracle, thirteen
wrong rules as named variants) and tests/test_gpu_cpic.py (the HIP kernels node by node and particle by particle).

Bounds are fixed multiples of u = 2^-24 times stated scales; the multiples were settled against the C fp32 oracle in
tests/test_cpic_truth.py, never against the kernels."""
from __future__ import annotations

import dataclasses
from typing import NamedTuple

import numpy as np

import cdf_truth as CT
import transfer_truth as T
from helpers import oracle, report_margin

U32, U64 = T.U32, T.U64
NONE = 0xFFFFFFFF
FRICTION = 20.0
NEAR_MAX = 0.05       # share of the particles near the speed cap or a threshold of sd (tests/test_gpu_transfer.py's NEAR_MAX)

# ---- fixed multiples of u
# velocity_at_point: the lever pt - com (1), the cross product (2 products and a difference per component, sqrt(D) in the
# norm: 3 sqrt(3) ~ 5), the sum with linvel (1): 8 of the scale |linvel| + |angvel| |pt - com|; an absolute error e of pt adds |angvel| e
C_BODY = 8.0
# project_velocity: n . v (2 D - 1 roundings), t = v - n (n . v) (2), |t| (D + 1), |t| + 20 (n . v) (2), t / |t| (1), the product (1):
# 16 for D = 3, of the scale L |v| with L its Lipschitz constant (below)
C_PROJ = 16.0
C_PEN = 8.0       # the penalty impulse: fl(0.3) fl(h), fl(dt), two products by 1e3 and dt, the product by n and the sum into v
C_THR = 4.0       # sd against fl(-0.05) fl(h) (and fl(-0.3) fl(h)): two roundings of the factors, one of the product, in units of u h
LEN_EPS = 1.0e-8  # project_velocity's |t| <= 1e-8 gives 0 instead of a vector no longer than |t|: the result moves by 1e-8 at most

VARIANTS = ("p2g_no_gate", "compat_ignores_sign", "g2p_incompatible_takes_grid", "ghost_no_projection", "body_vel_at_particle",
            "lever_from_translation", "angvel_cross_sign", "friction_1", "rigid_vel_lowest_bit", "pen_test_sd_lt_0", "no_clamp",
            "advect_after_penalty", "cap_before_projection")


# ------------------------------------------------------------------------------------------------ the rules
def compatible(a1, a2, variant=()):
    """affinities_are_compatible: the signs of the colliders both words carry agree"""
    a1, a2 = np.asarray(a1, np.uint32), np.asarray(a2, np.uint32)
    common = a1 & a2 & np.uint32(0xffff)
    if "compat_ignores_sign" in variant:
        return np.ones(np.broadcast(a1, a2).shape, bool)
    return ((a1 >> np.uint32(16)) & common) == ((a2 >> np.uint32(16)) & common)


def project_velocity(v, n, variant=()):
    """(out, branch) with branch 0: n . v >= 0 (unchanged), 1: stick (scale == 0), 2: slide"""
    f = 1.0 if "friction_1" in variant else FRICTION
    nv = np.einsum("...k,...k->...", v, n)
    t = v - n * nv[..., None]
    ln = np.linalg.norm(t, axis=-1)
    scale = np.maximum(0.0, ln + f * nv)
    with np.errstate(divide="ignore", invalid="ignore"):
        dirn = np.where((ln > LEN_EPS)[..., None], t / ln[..., None], 0.0)
    away = nv >= 0.0
    out = np.where(away[..., None], v, dirn * scale[..., None])
    return out, np.where(away, 0, np.where(scale > 0.0, 2, 1)), ln


def lipschitz(n):
    """of project_velocity in v: |dt| <= (1 + |n|^2) |dv|, the shrink t -> t max(0, 1 + c / |t|) is 1-Lipschitz in t and in
    c = 20 n . v, |dc| <= 20 |n| |dv|; the branches join continuously at n . v = 0 and at scale = 0"""
    nn = np.linalg.norm(n, axis=-1)
    return 1.0 + nn * nn + FRICTION * nn


class Motion:
    """linvel [nc, d], angvel [nc, 1 | 3], com, trans [nc, d] of the first min(16, n) colliders as fp64 of the fp32 values"""

    def __init__(self, linvel, angvel, com, trans):
        f = lambda a, k: CT.f32(np.asarray(a, np.float64).reshape(-1, k)) if len(a) else np.zeros((0, k))
        d = np.shape(trans)[1] if len(trans) else 2
        self.d = d
        self.linvel, self.com, self.trans = f(linvel, d), f(com, d), f(trans, d)
        self.angvel = f(angvel, 1 if d == 2 else 3)
        self.n = len(self.linvel)

    @staticmethod
    def of(colliders, d, poses=None):
        """of the scene's Collider records, or of read_body_poses() (taken before the substep)"""
        if poses is not None:
            g = lambda k: [np.asarray(p[k], np.float64) for p in poses]
            return Motion(g("linvel"), g("angvel"), g("com"), g("translation"))
        na = 1 if d == 2 else 3
        tr = [np.asarray(c.translation, np.float64)[:d] for c in colliders]
        return Motion([np.asarray(c.linvel, np.float64)[:d] for c in colliders],
                      [(np.asarray(list(c.angvel) + [0.0] * 3, np.float64))[:na] for c in colliders],
                      [t if c.com is None else np.asarray(c.com, np.float64)[:d] for c, t in zip(colliders, tr)], tr)

    def at(self, ids, pt, variant=()):
        """(velocity_at_point, its scale |linvel| + |angvel| |pt - com|, |angvel|) of colliders `ids` at points pt [..., d]"""
        com = self.trans if "lever_from_translation" in variant else self.com
        lever = pt - com[ids]
        w = -self.angvel[ids] if "angvel_cross_sign" in variant else self.angvel[ids]
        if self.d == 2:
            rot = np.stack([-w[..., 0] * lever[..., 1], w[..., 0] * lever[..., 0]], axis=-1)
        else:
            rot = np.cross(w, lever)
        an = np.linalg.norm(self.angvel[ids], axis=-1)
        return self.linvel[ids] + rot, np.linalg.norm(self.linvel[ids], axis=-1) + an * np.linalg.norm(lever, axis=-1), an


class Fields(NamedTuple):
    """the discrete decisions and the cdf of this substep (see the module docstring); nodes as arrays over world cells"""
    paff: np.ndarray
    pnormal: np.ndarray
    pdist: np.ndarray
    cells: np.ndarray
    naff: np.ndarray
    nclosest: np.ndarray


class Contact:
    """per particle: rigid_vel (the sum of velocity_at_point over the affinity bits c < min(16, n_colliders)) and the
    penetration branch of the particle update; what transfer_truth.Particles asks of its `contact`"""

    def __init__(self, inp, h, f: Fields, motion: Motion, u, variant=(), flip_near=False):
        n, d = inp.n, inp.d
        self.variant, self.h, self.u = variant, float(h), u
        self.normal = np.asarray(f.pnormal, np.float64)
        self.sd = np.asarray(f.pdist, np.float64)
        self.paff = paff = np.asarray(f.paff, np.uint32)
        self.rigid_vel = np.zeros((n, d))
        scale = np.zeros(n)
        bits = np.zeros(n)
        done = np.zeros(n, bool)
        for c in range(min(16, motion.n)):
            has = ((paff >> np.uint32(c)) & 1).astype(bool)
            if "rigid_vel_lowest_bit" in variant:
                has &= ~done
                done |= has
            if has.any():
                v, s, _ = motion.at(np.full(int(has.sum()), c), inp.x[has], variant)
                self.rigid_vel[has] += v
                scale[has] += s
                bits[has] += 1.0
        # each term C_BODY u of its scale (x is given: no error of the point), each of the sums one more u of the partial sums
        self.b_rigid = u * (C_BODY + bits) * scale
        thr = 0.0 if "pen_test_sd_lt_0" in variant else -0.05 * self.h
        self.pen = self.sd < thr
        self.near_pen = np.abs(self.sd + 0.05 * self.h) <= C_THR * u * self.h
        self.near_clamp = np.abs(self.sd + 0.3 * self.h) <= C_THR * u * self.h
        if flip_near:                                     # the other side of the threshold for the particles near it
            self.pen = self.pen ^ self.near_pen
        self.branch = np.full(n, -1)

    @property
    def near(self):
        return self.near_pen | self.near_clamp

    def project(self, v, b, u):
        """rigid_vel + project_velocity(v - rigid_vel, normal) where sd < -0.05 h"""
        rel = v - self.rigid_vel
        out, br, ln = project_velocity(rel, self.normal, self.variant)
        rn = np.linalg.norm(rel, axis=1)
        L = lipschitz(self.normal)
        # the difference carries both errors and its own rounding; the projection magnifies them by L and adds C_PROJ u L |rel|;
        # the sum with rigid_vel its error again and one rounding
        bo = L * (b + self.b_rigid + u * rn) + C_PROJ * u * L * rn + np.where(ln <= 2.0 * LEN_EPS, 2.0 * LEN_EPS, 0.0)
        new = self.rigid_vel + out
        self.branch = np.where(self.pen, br, -1)
        return np.where(self.pen[:, None], new, v), np.where(self.pen, bo + self.b_rigid + u * np.linalg.norm(new, axis=1), b)

    def penalty(self, dt, u):
        """dt * -max(sd, -0.3 h) * 1e3 * normal where sd < -0.05 h"""
        corr = self.sd if "no_clamp" in self.variant else np.maximum(self.sd, -0.3 * self.h)
        imp = np.where(self.pen, dt * -corr * 1.0e3, 0.0)
        nn = np.linalg.norm(self.normal, axis=1)
        # (near the clamp the two sides differ by C_THR u h dt 1e3 |n| at most: the clamp is continuous)
        b = C_PEN * u * np.abs(imp) * nn + np.where(self.near_clamp & self.pen, C_THR * u * self.h * dt * 1.0e3 * nn, 0.0)
        return imp[:, None] * self.normal, b


class Result(NamedTuple):
    st: T.Stencil
    grid: T.Grid                   # gated P2G + grid update; .dimp [M, d]: the momentum not transferred, .pairs: its pairs (checked by tests/body_truth.py)
    particles: T.Particles
    contact: Contact
    compat: np.ndarray             # [n, S] pairs that transfer
    ghost_branch: np.ndarray       # [n, S] -1: compatible, 0 / 1 / 2: project_velocity's branch, 3: no collider (the particle's own velocity)
    nclosest: np.ndarray           # [n, S]
    other: object = None           # the Particles with the particles near sd = -0.05 h on the other side of it (None: no such particle)


def _stencil_fields(st, f: Fields, d):
    keys = T.node_key(np.asarray(f.cells, np.int64))
    order = np.argsort(keys)
    sk = keys[order]
    want = T.node_key(st.node.reshape(-1, d))
    j = np.minimum(np.searchsorted(sk, want), max(len(sk) - 1, 0))
    hit = (sk[j] == want) if len(sk) else np.zeros(len(want), bool)
    S = st.w.shape[1]
    naff = np.where(hit, np.asarray(f.naff, np.uint32)[order][j], 0).astype(np.uint32).reshape(-1, S)
    ncl = np.where(hit, np.asarray(f.nclosest, np.uint32)[order][j], NONE).astype(np.uint32).reshape(-1, S)
    return naff, ncl


def substep(inp: T.Inputs, h, dt, gravity, f: Fields, motion: Motion, variant=(), u=U32, extra_levels=0.0, own_grid=None):
    """The fp64 CPIC substep from the given decisions. End to end (the node bounds of a kernel of unit roundoff u propagated
    into the particle bounds), or with `own_grid` = (cells [M, d], velocities [M, d]) of a kernel's read-back grid: the
    isolated G2P truth (compatible pairs read that grid as exact; ghost velocities are computed either way)."""
    d = inp.d
    st = T.Stencil(inp, h)
    naff, ncl = _stencil_fields(st, f, d)
    paff = np.asarray(f.paff, np.uint32)
    normal = np.asarray(f.pnormal, np.float64)
    compat = compatible(paff[:, None], naff, variant)
    gr = T.Grid(inp, st, dt, gravity, gate=None if "p2g_no_gate" in variant else compat)
    # ---- the ghost velocity of every incompatible pair
    S = st.w.shape[1]
    node_vel = np.broadcast_to(inp.v[:, None, :], (inp.n, S, d)).copy()     # (no collider: the particle's own velocity, exact)
    node_b = np.zeros((inp.n, S))
    branch = np.where(compat, -1, 3)
    p, s = np.nonzero(~compat & (ncl < motion.n))
    if len(p):
        cc = inp.x[p] + st.dpt[p, s]
        at = inp.x[p] if "body_vel_at_particle" in variant else cc
        bv, bscale, an = motion.at(ncl[p, s].astype(np.int64), at, variant)
        rel = inp.v[p] - bv
        if "ghost_no_projection" in variant:
            out, br, ln = rel, np.zeros(len(p), int), np.full(len(p), np.inf)
        else:
            out, br, ln = project_velocity(rel, normal[p], variant)
        ghost = bv + out
        node_vel[p, s] = ghost
        branch[p, s] = br
        # the point x + dpt carries dpt's error and its own rounding: |angvel| of it in the body velocity
        b_bv = C_BODY * u * bscale + an * u * (st.dpt_error[p] + np.linalg.norm(cc, axis=1))
        rn = np.linalg.norm(rel, axis=1)
        L = lipschitz(normal[p])
        node_b[p, s] = b_bv + L * (b_bv + u * rn) + C_PROJ * u * L * rn + np.where(ln <= 2.0 * LEN_EPS, 2.0 * LEN_EPS, 0.0) + \
            u * np.linalg.norm(ghost, axis=1)
        # the momentum a pair does not transfer: what the closest body receives (tests/body_truth.py reads the pairs)
        dimp = (inp.v[p] - ghost) * (st.w[p, s] * inp.m[p])[:, None]
        gr.dimp = np.stack([np.bincount(gr.inv[p, s], dimp[:, k], len(gr.keys)) for k in range(d)], 1)
        gr.pairs = (p, s, ghost, node_b[p, s])
    else:
        gr.dimp = np.zeros((len(gr.keys), d))
        gr.pairs = (p, s, np.zeros((0, d)), np.zeros(0))
    takes_grid = compat | ("g2p_incompatible_takes_grid" in variant)
    if own_grid is None:
        _, bv_n, _ = gr.bounds(u, extra_levels)
        gv, gb = gr.vel[gr.inv], bv_n[gr.inv]
    else:
        cells, vel = own_grid
        keys = T.node_key(cells)
        order = np.argsort(keys)
        sk = keys[order]
        want = T.node_key(st.node.reshape(-1, d))
        i = np.minimum(np.searchsorted(sk, want), len(sk) - 1)
        assert np.array_equal(sk[i], want), "a stencil node of a particle is missing from the grid"
        gv, gb = np.asarray(vel, np.float64)[order][i].reshape(inp.n, S, d), np.zeros((inp.n, S))
    node_vel = np.where(takes_grid[..., None], gv, node_vel)
    node_b = np.where(takes_grid, gb, node_b)
    ct = Contact(inp, h, f, motion, u, variant)
    pt = T.Particles(inp, st, node_vel, dt, node_bound=node_b, u=u, contact=ct)
    other = None
    if ct.near_pen.any():
        other = T.Particles(inp, st, node_vel, dt, node_bound=node_b, u=u, contact=Contact(inp, h, f, motion, u, variant, flip_near=True))
    return Result(st, gr, pt, ct, compat, branch, ncl, other)


# ------------------------------------------------------------------------------------------------ checks
def excess(res: Result, cells, vm, got, model, u=U32, extra_levels=0.0):
    """error / bound of every checked element by check name (near particles left out; a node of zero truth mass that holds
    a value: inf): what the variant tests count"""
    gr, pt, d = res.grid, res.particles, res.grid.d
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        if cells is not None:
            vm = np.asarray(vm, np.float64)
            i = gr.lookup(cells)
            zero = (i < 0) | (gr.mass[np.maximum(i, 0)] == 0.0)
            j = i[~zero]
            bm, bv, _ = gr.bounds(u, extra_levels)
            out["zero nodes"] = np.where(np.abs(vm[zero]).max(1) != 0.0, np.inf, 0.0) if zero.any() else np.zeros(0)
            out["node mass"] = np.abs(vm[~zero, d] - gr.mass[j]) / bm[j]
            out["node velocity"] = np.linalg.norm(vm[~zero, :d] - gr.vel[j], axis=1) / bv[j]
        keep = ~res.contact.near_pen
        for k, r in zip(("x", "v", "F", "C'"), _ratios(pt, got, model)):
            out[k] = r[keep]
    return {k: np.where(np.isnan(v), 0.0, v) for k, v in out.items()}


def _ratios(pt, got, model):
    """error / bound of x, v, F, C' of every particle"""
    g = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    f = lambda k: np.asarray(g(k), np.float64)
    d = pt.d
    Cn, bC = pt.affine(model, f("def_grad"))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = [np.linalg.norm(f("pos") - pt.x, axis=1) / pt.b_x, np.linalg.norm(f("vel") - pt.vel, axis=1) / pt.b_vel,
               np.linalg.norm(T.mat(f("def_grad"), d) - pt.F, axis=(1, 2)) / pt.b_F, np.linalg.norm(T.mat(f("affine"), d) - Cn, axis=(1, 2)) / bC]
    return [np.where(np.isnan(r), 0.0, r) for r in out]


def check_result(tag, res: Result, cells, vm, got, model, fails, u=U32, extra_levels=0.0, sel=None):
    """transfer_truth's checks of the grid (cells None: particles only) and of the particles that are not near the
    threshold sd = -0.05 h; those that are must fit one of its two sides; cdf_rigid_vel where `got` has it; returns (near
    nodes, nodes, near particles)"""
    near_n = nn = 0
    if cells is not None:
        near_n, nn = T.check_grid(f"{tag} grid", res.grid, cells, vm, fails, u=u, extra_levels=extra_levels)
    ct = res.contact
    keep = ~ct.near_pen if sel is None else (~ct.near_pen & sel)
    T.check_particles(tag, res.particles, got, model, fails, sel=keep)
    nearp = ct.near_pen if sel is None else (ct.near_pen & sel)
    if nearp.any():                                       # either side of sd = -0.05 h is accepted: all of x, v, F, C' of one of them
        fit = [np.all([r <= 1.0 for r in _ratios(p, got, model)], axis=0) for p in (res.particles, res.other)]
        bad = nearp & ~(fit[0] | fit[1])
        report_margin(f"{tag}: particles near sd = -0.05 h that fit neither side", int(bad.sum()), 0, n=int(nearp.sum()))
        if bad.any():
            fails.append(f"{tag}: {int(bad.sum())} of {int(nearp.sum())} particles near sd = -0.05 h fit neither side (first #{int(np.argmax(bad))})")
    rv = got.get("cdf_rigid_vel") if isinstance(got, dict) else getattr(got, "cdf_rigid_vel", None)
    if rv is not None:
        # (exactly 0 where the particle carries no affinity bit of a collider: nothing is summed)
        T.check(f"{tag}: rigid_vel (scale sum |linvel| + |angvel| |x - com|)", np.linalg.norm(np.asarray(rv, np.float64) - ct.rigid_vel, axis=1),
                ct.b_rigid, fails, sel)
    near = res.particles.near_cap | res.contact.near
    return near_n, nn, int((near if sel is None else near & sel).sum())


def assert_near(tag, near_n, nn, near_p, n):
    report_margin(f"{tag}: nodes near the clamp (fraction)", near_n / max(nn, 1), NEAR_MAX, count=near_n)
    report_margin(f"{tag}: particles near the speed cap or a threshold of sd (fraction)", near_p / max(n, 1), NEAR_MAX, count=near_p)
    assert near_n <= NEAR_MAX * nn and near_p <= NEAR_MAX * n, (tag, near_n, nn, near_p, n)


def reach(res: Result):
    """the counts the scenes are built for"""
    ct, gr = res.contact, res.grid
    inc = ~res.compat
    paff = ct.paff
    nbits = np.zeros(len(paff), int)
    for c in range(16):
        nbits += ((paff >> np.uint32(c)) & 1).astype(int)
    reached = np.bincount(gr.inv.reshape(-1), None, len(gr.keys))
    br = np.concatenate([res.ghost_branch[inc & (res.ghost_branch < 3)], ct.branch[ct.pen]])
    return dict(incompatible_pairs=int(inc.sum()), particles_with_incompatible=int(inc.any(1).sum()),
                multi_affinity=int((nbits >= 2).sum()), only_incompatible_nodes=int(((reached > 0) & (gr.count == 0)).sum()),
                penetrating=int(ct.pen.sum()), deeper_than_clamp=int((ct.pen & (ct.sd < -0.3 * ct.h)).sum()),
                away=int((br == 0).sum()), stick=int((br == 1).sum()), slide=int((br == 2).sum()),
                closest_ids=sorted(set(np.unique(res.nclosest[inc]).tolist()) - {NONE}))


# ------------------------------------------------------------------------------------------------ scenes
def moving(col, i, d, h, speed=1.0):
    """collider i in motion: every velocity component non-zero, |linvel| <= 0.1 h / dt (times `speed`) and |angvel| <= 1 (what
    a body in contact is capped to), the centre of mass off the translation"""
    s = (-1.0 if i % 2 else 1.0) * (1.0 - 0.03 * i)
    lin = np.array([0.7, -0.4, 0.5]) * (0.1 * h / T.DT * s * speed)
    if d == 2:
        lin[2] = 0.0
    ang = (0.8 * s,) if d == 2 else tuple(np.array([0.5, -0.6, 0.4]) * s)
    com = np.zeros(3)
    com[:d] = np.asarray(col.translation, np.float64)[:d] + (np.array([0.6, -0.3, 0.4]) * h)[:d]
    f = lambda a: tuple(float(v) for v in CT.f32(a))
    return dataclasses.replace(col, linvel=f(lin), angvel=f(ang), com=f(com[:d]))


def plate(d, h, seed=8, **kw):
    """a thin plate (half thickness 0.3 h) with particles on both sides"""
    from wgsparkl_amd.solver import Collider
    rng = np.random.default_rng(seed)
    x0 = np.array([4.13, 6.21, 6.17]) * h
    cols = [Collider.cuboid(CT._v(np.array([0.3, 3.0, 3.0]) * h, d), CT._v(x0, d), rotation=CT.ident(d))]
    lo, hi = np.array([1.0, 3.5, 3.5]) * h, np.array([7.3, 9.0, 9.0]) * h
    return CT._static(d, h, rng, cols, [(lo, hi)], 3000 if d == 3 else 1500, **kw)


_STATIC = dict(cuboid=CT.cuboid, capsule=CT.capsule, two_equal=CT.two_equal, ball=CT.ball, sixteen=CT.sixteen, plate=plate)
# Every bound of a particle in contact is a multiple of u L^2 (|v_p| + |body velocity|): the ghost velocities' errors pass
# through project_velocity (L ~ 22) in G2P and again in the update. At 0.1 h / dt that is ~0.3 h / s, as much as the whole
# penalty impulse (<= 0.3 h / s), so a wrong penalty rule hides in it: the plate scene moves at a fiftieth of that speed.
SPEED = dict(plate=0.02)
TANGENTIAL = 0.3      # share of the particles near a collider whose relative velocity is set near-tangential


def _scene(name):
    def build(d, h, model=0, uniform=False, prev=True, fixed=False):
        """the cdf_truth scene `name` stirred: particle velocities N(0, 0.1 h / dt) per axis (times SPEED[name]), a random C, F near I, gravity
        with every component non-zero, every collider in motion (`moving`), the previous affinity words of cdf_truth._prev
        uploaded (a third carry collider 0 positive, a third negative: particles on either side of sd = -0.05 h and of
        -0.3 h by their own stored sign), and a subset of the particles near a collider whose velocity relative to it is
        near-tangential (|normal part| = 1/40 of the tangential part, speeds 0.02 .. 4 h / dt times SPEED[name]: both sides of
        the speed cap in every scene but the slow one). `fixed`: the colliders stay at rest (no collider has a velocity or a mass:
        the library then runs the one-way P2G); ghost velocities are still non-zero through the particles' own."""
        make = _STATIC[name]
        case = CT._case(make, d, h)                           # (positions, previous words and the cdf truth: built once)
        sc = dict(make(d, h, uniform=uniform))
        ps = sc["particles"]
        assert np.array_equal(ps.pos, case.sc["particles"].pos)
        rng = np.random.default_rng(1000 + 10 * d + int(10 * h))
        n = ps.n
        s = 0.1 * h / T.DT * SPEED.get(name, 1.0)
        vel = rng.normal(0.0, s, (n, d))
        cols = list(sc["colliders"]) if fixed else [moving(c, i, d, h, SPEED.get(name, 1.0)) for i, c in enumerate(sc["colliders"])]
        mo = Motion.of(cols, d)
        pf = case.truth.particles
        nrm = pf.normal
        nn = np.linalg.norm(nrm, axis=1)
        low = np.zeros(n, np.int64)
        for c in range(15, -1, -1):
            low = np.where(((pf.aff >> np.uint32(c)) & 1).astype(bool), c, low)
        pick = np.nonzero((pf.aff != 0) & (nn > 0.5) & (low < mo.n) & (rng.random(n) < TANGENTIAL))[0]
        if len(pick):
            nh = nrm[pick] / nn[pick, None]
            t = rng.normal(0.0, 1.0, (len(pick), d))
            t -= nh * np.einsum("nk,nk->n", t, nh)[:, None]
            t /= np.linalg.norm(t, axis=1)[:, None]
            speed = s * 10.0 ** rng.uniform(np.log10(0.2), np.log10(40.0), len(pick))
            bv = mo.at(low[pick], ps.pos[pick].astype(np.float64))[0]
            vel[pick] = bv + (t - nh / 40.0) * speed[:, None]
        ps.vel[:] = vel.astype(np.float32)
        ps.affine[:] = (rng.normal(0.0, s / h, (n, d * d)) * ps.mass[:, None]).astype(np.float32)
        ps.def_grad[:] = (np.eye(d).reshape(-1) + rng.normal(0.0, 0.01, (n, d * d))).astype(np.float32)
        if prev:
            ps.cdf_affinity[:] = case.prev
        from wgsparkl_amd.solver import SimulationParams
        sc.update(params=SimulationParams(gravity=T.GRAVITY[:d], dt=T.DT), colliders=cols, model=model)
        return sc
    build.__name__ = name
    return build


SCENES = {name: _scene(name) for name in _STATIC}
HS = CT.HS


# ------------------------------------------------------------------------------------------------ the C oracle beside the truth
class OracleRun(NamedTuple):
    fields: Fields                 # the oracle's own cdf fields of the substep
    cells: np.ndarray
    vm: np.ndarray                 # node velocity | mass after the grid update
    arr: dict                      # the particles after the substep


def oracle_substep(sc, dtype):
    """One substep of the C oracle pass by pass in the order of orc_step_full, without the bodies' integration at its end;
    the previous affinity words are the particles' own (ps.cdf_affinity)."""
    ps = sc["particles"]
    st = oracle(ps.dim, dtype).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc.get("model", 0))
    st.update_rigid_particles()
    st.sort_rigid()
    assert not st.overflow
    st.grid_update_cdf()
    st.p2g_cdf()
    st.g2p_cdf()
    st.g["impulses"][:] = 0
    st.p2g()
    st.grid_update()
    st.g2p()
    st.particle_update()
    cells, mv, _, aff, closest = st.grid_records()
    f = Fields(st.arr["cdf_affinity"].copy(), st.arr["cdf_normal"].astype(np.float64), st.arr["cdf_dist"].astype(np.float64), cells, aff, closest)
    return OracleRun(f, cells, np.asarray(mv, np.float64), {k: v.copy() for k, v in st.arr.items()})
