"""fp64 truth of one collider-free substep (P2G, grid update, G2P, particle update) from fp32 inputs, with the per-element
scales that a rounding bound needs, and the bounds themselves. Shared by tests/test_transfer_truth.py (CPU: the truth
against the C fp64 oracle, the bounds against the C fp32 oracle and against perturbations of it) and
tests/test_gpu_transfer.py (the HIP kernels node by node and particle by particle).

Written from oracle/np_oracle.py (same formulas, vectorised, fp64) with the kernels' roundings in mind:
- the associated cell is the bit-exact fp32 rule round(x / h) - 1 (np_oracle.assoc_cell), so truth and kernel use the
  same stencil; the weights and dpt are then evaluated in fp64 from the fp32 position and h;
- a kernel's weight carries an absolute error that grows with |cell|: ref = cell * h - x cancels, and cell * h is rounded
  (and h itself is the fp32 h). That error is a stated per-particle scale (`weight_error`), in units of u.

Bounds follow tests/test_gpu_devmath.py: fixed multiples of u = 2^-24 times stated scales; for a node, the multiple grows
linearly in its number of contributors (the summation depth). The clamp of the grid velocity at +-h/dt and the speed cap
at h/dt are 1-Lipschitz maps, so a bound on the value before them bounds the value after them; elements whose truth lies
within its bound of a clamp are counted (either side is then a legitimate outcome) and their fraction is reported."""
from __future__ import annotations

import numpy as np

import devmath_truth as DM
from helpers import report_margin
from oracle.np_oracle import assoc_cell, bw_of, eval_all, mat64 as mat, shifts_of, unmat

U32 = 2.0 ** -24
U64 = 2.0 ** -53
NEAR_CLAMP = 1.0e-5       # relative distance to h/dt inside which the fp32 h/dt (or h, dt) may put a value on either side
LOOSE = 0.01              # a bound above this fraction of h/dt says little about the clamp: not counted as near it

# fixed multiples of u (each bound below says which scale it multiplies)
C_ACC = 2.0      # node sums, per contributor: term (two roundings) + one addition; the tile / wave / gather levels are C_LVL
C_LVL = 32.0     # the summation levels above the per-cell runs: 9 tile phases, 4 wave tiles, 2^D source slabs, shard halves
C_WT = 4.0       # a weight's absolute error per unit of `weight_error` (see there)
C_GU = 8.0       # grid update: (p + m g dt) / m and the inverse
C_G2P = 32.0     # G2P: 3^D weighted terms through the tensor-product evaluation (x, then y, then z)
C_UPD = 8.0      # particle update: cap, x + v dt, F + (grad dt) F, grad m - tau c


def node_key(cells):
    """int64 key of world node coordinates (|cell| < 2^20 per axis)"""
    c = np.asarray(cells, np.int64) + (1 << 20)
    k = c[:, 0]
    for j in range(1, c.shape[1]):
        k = (k << 21) | c[:, j]
    return k


class Inputs:
    """fp32 particle state of one substep, as fp64 arrays (matrices [n, row, col])."""

    def __init__(self, pos, vel, affine, def_grad, mass, init_volume, lambda_, mu):
        self.pos32 = np.ascontiguousarray(pos, np.float32)
        self.n, self.d = self.pos32.shape
        d = self.d
        f = lambda a: np.asarray(np.asarray(a, np.float32), np.float64)
        self.x, self.v = f(pos), f(vel)
        self.C, self.F = mat(f(affine), d), mat(f(def_grad), d)
        self.m, self.vol, self.lam, self.mu = f(mass), f(init_volume), f(lambda_), f(mu)

    @staticmethod
    def of(ps):
        """from a ParticleSet or an oracle state's `arr` dict"""
        g = (lambda k: ps[k]) if isinstance(ps, dict) else (lambda k: getattr(ps, k))
        return Inputs(g("pos"), g("vel"), g("affine"), g("def_grad"), g("mass"), g("init_volume"), g("lambda_"), g("mu"))


class Stencil:
    """weights, dpt and nodes of every particle (fp64 from the fp32 positions, bit-exact cells)"""

    def __init__(self, inp: Inputs, h: float, variant=()):
        d = inp.d
        self.h = float(h)
        cell = assoc_cell(inp.pos32, h)
        ref = cell * self.h - inp.x                                      # [n, d]
        t = -ref * self.h if "p2g_ref_times_h" in variant else -ref / self.h
        w = eval_all(t)                                                  # [n, d, 3]
        sh = shifts_of(d)
        self.w = np.ones((inp.n, len(sh)))
        for k in range(d):
            self.w *= w[:, k, sh[:, k]]
        self.ref = ref
        self.dpt = ref[:, None, :] + sh[None, :, :] * self.h             # [n, S, d]
        self.node = cell[:, None, :] + sh[None, :, :]                    # [n, S, d]
        # Absolute error of a kernel's weight, in units of u: t = -(cell h - x) / h carries ~2 |cell| u from cell * h
        # (rounded, and with the fp32 h) unless h is a power of two (then cell * h and the subtraction are exact), plus a
        # few u from the subtraction, the multiplication by 1/h and eval_all; the product of d factors adds them up.
        far = (0.0 if _pow2(self.h) else 2.0) * np.abs(cell).max(1)
        self.weight_error = d * (far + 8.0)                              # [n]
        self.dpt_error = self.h * (far + 8.0)                           # absolute error of dpt, units of u


class Grid:
    """fp64 P2G + grid update. Node arrays are over the unique stencil nodes (`cells`, sorted by key)."""

    def __init__(self, inp: Inputs, st: Stencil, dt, gravity, variant=(), gate=None):
        """`gate` [n, S] bool (CPIC, tests/cpic_truth.py): the (particle, node) pairs that transfer; the others add nothing to a
        node, and are not among its contributors. None: every pair transfers."""
        d = inp.d
        h = st.h
        sw = st.w if gate is None else np.where(gate, st.w, 0.0)
        g = np.zeros(d)
        g[:] = np.asarray(gravity, np.float64)[:d]
        if "gravity_g1_on_every_axis" in variant:
            g[:] = g[1]
        self.d, self.h, self.dt, self.g = d, h, float(dt), g
        self.lim = 1.0 / self.dt if "grid_clamp_inv_dt" in variant else h / self.dt
        keys = node_key(st.node.reshape(-1, d))
        self.keys, first, inv = np.unique(keys, return_index=True, return_inverse=True)
        self.cells = st.node.reshape(-1, d)[first]
        self.inv = inv.reshape(inp.n, -1)                                # particle stencil slot -> node index
        M = len(self.keys)
        mv = inp.m[:, None] * inp.v                                       # [n, d]
        cd = np.einsum("nrc,nsc->nsr", inp.C, st.dpt)                     # [n, S, d]
        mom = cd + mv[:, None, :]
        idx = self.inv.reshape(-1)
        wm = (inp.m[:, None] * sw).reshape(-1)
        self.mass = np.bincount(idx, wm, M)
        self.mom = np.stack([np.bincount(idx, (mom[..., k] * sw).reshape(-1), M) for k in range(d)], 1)
        self.count = np.bincount(idx, None if gate is None else gate.reshape(-1).astype(np.float64), M)
        # scales: sum w m, sum w |m v + C dpt| (as |m v| + |C| |dpt|: what the kernel rounds), and the weight-error sums
        cn = np.linalg.norm(inp.C, axis=(1, 2))
        amom = np.linalg.norm(mv, axis=1)[:, None] + cn[:, None] * np.linalg.norm(st.dpt, axis=2)
        self.s_m = self.mass.copy()
        self.s_p = np.bincount(idx, (sw * amom).reshape(-1), M)
        ew = st.weight_error[:, None] * (np.ones_like(st.w) if gate is None else gate.astype(np.float64))
        self.e_m = np.bincount(idx, (ew * inp.m[:, None]).reshape(-1), M)
        self.e_p = np.bincount(idx, (ew * amom + sw * (cn * st.dpt_error)[:, None]).reshape(-1), M)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv_m = np.where(self.mass > 0, 1.0 / self.mass, 0.0)
        self.vel_u = (self.mom + self.mass[:, None] * g[None, :] * self.dt) * inv_m[:, None]
        self.vel = np.clip(self.vel_u, -self.lim, self.lim)

    def bounds(self, u=U32, extra_levels=0.0):
        """(mass bound, velocity bound per node [normwise over the d components], near-clamp flags) for a kernel of
        unit roundoff u. Velocity: first order in the mass and momentum errors while they are below half the mass,
        otherwise any clamped value (2 sqrt(d) lim)."""
        n = self.count
        acc = u * (C_ACC * n + C_LVL + extra_levels)
        bm = acc * self.s_m + C_WT * u * self.e_m
        bp = acc * self.s_p + C_WT * u * self.e_p
        M = self.mass
        vu = np.linalg.norm(self.vel_u, axis=1)
        gdt = np.linalg.norm(self.g) * self.dt
        anyv = 2.0 * np.sqrt(self.d) * self.lim
        with np.errstate(divide="ignore", invalid="ignore"):
            first = 2.0 * (bp + bm * (vu + gdt)) / M + C_GU * u * (self.s_p / M + vu + gdt)
        bv = np.where((M > 0) & (bm < 0.5 * M), np.minimum(first, anyv), anyv)
        # near the clamp: decided to within the bound, the bound itself well below h / dt (elsewhere the node is loose:
        # its weights' error is comparable to its mass, far from the origin or at the tails of the stencil)
        near = np.any(np.abs(np.abs(self.vel_u) - self.lim) <= bv[:, None] + NEAR_CLAMP * self.lim, axis=1) & (M > 0) & \
            (bv < LOOSE * self.lim)
        bv = bv + np.where(np.any(np.abs(self.vel_u) >= self.lim * (1.0 - NEAR_CLAMP), axis=1), 4.0 * u * self.lim, 0.0)
        return bm, np.minimum(bv, anyv), near

    def lookup(self, cells):
        """node indices of world cells (-1: no particle reaches the node)"""
        k = node_key(cells)
        i = np.searchsorted(self.keys, k)
        i = np.minimum(i, len(self.keys) - 1)
        return np.where(self.keys[i] == k, i, -1)


class Particles:
    """fp64 G2P + particle update (no colliders, elastic) from given node velocities, with per-particle bounds.

    `node_vel` [n, S, d]: the velocity of every stencil node of every particle (fp64 truth grid, or a kernel's own grid:
    the isolated G2P truth). `node_bound` [n, S]: the bound of those node velocities (0 for a kernel's own grid)."""

    def __init__(self, inp: Inputs, st: Stencil, node_vel, dt, node_bound=None, u=U32, variant=(), contact=None):
        """`contact` (CPIC, a cpic_truth.Contact): project(vel_g, b_vel_g, u) -> (velocity, bound) of the penetrating particles'
        projection before the speed cap, penalty(dt, u) -> (dv, bound) of the impulse added after the advection; its
        variants "cap_before_projection" and "advect_after_penalty" reorder the update. None: no collider."""
        d, h, dt = inp.d, st.h, float(dt)
        self.d, self.h, self.dt, self.u = d, h, dt, u
        self.lim = h / dt
        self.inp, self.st = inp, st
        w = st.w
        self.invd = 4.0 if "invd_4" in variant else 4.0 / (h * h)
        self.vel_g = np.einsum("ns,nsr->nr", w, node_vel)
        self.grad = self.invd * np.einsum("ns,nsr,nsc->nrc", w, node_vel, st.dpt)
        # ---- bounds (normwise per particle)
        anv = np.linalg.norm(node_vel, axis=2)                            # [n, S]
        s_v = np.einsum("ns,ns->n", w, anv)
        ew = C_WT * u * st.weight_error
        dn = np.linalg.norm(st.dpt, axis=2)
        rn = np.linalg.norm(st.ref, axis=1)
        b_vel = C_G2P * u * s_v + ew * anv.sum(1)
        b_grad = self.invd * (C_G2P * u * s_v * (rn + 2.0 * h) + ew * (anv * dn).sum(1) + C_WT * u * s_v * st.dpt_error)
        if node_bound is not None:
            b_vel = b_vel + np.einsum("ns,ns->n", w, node_bound)
            b_grad = b_grad + self.invd * np.einsum("ns,ns,ns->n", w, node_bound, dn)
        self.b_vel_g = b_vel
        cvar = () if contact is None else contact.variant
        pre = self.vel_g
        if "cap_before_projection" in cvar:
            s0 = np.linalg.norm(pre, axis=1)
            pre = np.where((s0 > self.lim)[:, None], pre * (self.lim / np.maximum(s0, 1e-300))[:, None], pre)
        if contact is not None:
            pre, b_vel = contact.project(pre, b_vel, u)
        self.vel_c = pre
        speed = np.linalg.norm(pre, axis=1)
        cap = (speed > self.lim) & ("cap_before_projection" not in cvar)
        self.vel = pre.copy()
        self.vel[cap] *= (self.lim / speed[cap])[:, None]
        self.near_cap = (np.abs(speed - self.lim) <= b_vel + NEAR_CLAMP * self.lim) & (b_vel < LOOSE * self.lim)
        self.b_vel = b_vel + C_UPD * u * np.linalg.norm(self.vel, axis=1) + np.where(speed >= self.lim * (1 - NEAR_CLAMP), 4 * u * self.lim, 0.0)
        self.b_grad = b_grad
        vn = np.linalg.norm(self.vel, axis=1)
        self.vel_adv = self.vel
        b_adv = self.b_vel
        if contact is not None:
            dv, b_dv = contact.penalty(dt, u)
            self.vel = self.vel + dv
            self.b_vel = self.b_vel + b_dv
            if "advect_after_penalty" in cvar:
                self.vel_adv = self.vel
        self.x = inp.x + self.vel_adv * dt
        self.F = inp.F + (self.grad * dt) @ inp.F
        self.b_x = dt * b_adv + C_UPD * u * (np.linalg.norm(inp.x, axis=1) + dt * vn)
        fn = np.linalg.norm(inp.F, axis=(1, 2))
        gn = np.linalg.norm(self.grad, axis=(1, 2))
        self.b_F = dt * b_grad * fn + C_UPD * u * d * (fn + dt * gn * fn)

    def affine(self, model, F_used):
        """C' = grad m - tau(F_used) V0 (4 / h^2) dt with tau in fp64 from the given F' (a kernel's own F': the stress of
        another F is checked by test_gpu_devmath), and its bound with devmath_truth's stress scale."""
        inp, u = self.inp, self.u
        Fu = mat(F_used, self.d) if np.ndim(F_used) == 2 else np.asarray(F_used, np.float64)
        if model == 0:
            U, s, V = DM.svd_lapack(unmat(Fu))
            tau = DM.tau_corotated64(Fu, inp.lam, inp.mu, U, s)
        else:
            s = np.linalg.svd(Fu, compute_uv=False)
            tau = DM.tau_neo_hookean64(Fu, inp.lam, inp.mu)
        coeff = inp.vol * self.invd * self.dt
        Cn = self.grad * inp.m[:, None, None] - tau * coeff[:, None, None]
        gn = np.linalg.norm(self.grad, axis=(1, 2))
        tn = np.linalg.norm(tau, axis=(1, 2))
        b = inp.m * self.b_grad + coeff * DM.C_TAU * u * DM.tau_scales(model, Fu, inp.lam, inp.mu, s) + \
            C_UPD * u * (inp.m * gn + coeff * tn)
        return Cn, b


def substep(inp: Inputs, h, dt, gravity, variant=(), u=U32, extra_levels=0.0):
    """(Stencil, Grid, Particles) of the fp64 substep: the end-to-end truth, with the node bounds (of a kernel of unit
    roundoff u) propagated into the particle bounds."""
    st = Stencil(inp, h, variant)
    gr = Grid(inp, st, dt, gravity, variant)
    _, bv, _ = gr.bounds(u, extra_levels)
    pt = Particles(inp, st, gr.vel[gr.inv], dt, node_bound=bv[gr.inv], u=u, variant=variant)
    return st, gr, pt


def isolated(inp: Inputs, st: Stencil, cells, node_vel, dt, variant=(), u=U32):
    """G2P truth from a kernel's own node velocities (cells [M, d] with velocities [M, d], the read-back grid): a G2P
    error is then separated from a P2G one. Stencil nodes that are not in the read-back grid are an error."""
    keys = node_key(cells)
    order = np.argsort(keys)
    sk = keys[order]
    want = node_key(st.node.reshape(-1, inp.d))
    i = np.minimum(np.searchsorted(sk, want), len(sk) - 1)
    assert np.array_equal(sk[i], want), "a stencil node of a particle is missing from the grid"
    nv = np.asarray(node_vel, np.float64)[order][i].reshape(inp.n, -1, inp.d)
    return Particles(inp, st, nv, dt, u=u, variant=variant)


# ------------------------------------------------------------------------------------------------ checks
def check(tag, err, bound, fails, sel=None):
    """per-element err <= bound (both [n]); reports the worst margin; appends a failure message"""
    err = np.asarray(err, np.float64)
    bound = np.asarray(bound, np.float64)
    if sel is not None:
        idx = np.nonzero(sel)[0]
        err, bound = err[sel], bound[sel]
    else:
        idx = np.arange(len(err))
    if not err.size:
        return
    ok = np.isfinite(err) & (err <= bound)
    r = np.where(bound > 0, err / np.maximum(bound, 1e-300), np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isfinite(err), r, np.inf)
    wi = int(np.argmax(r))
    report_margin(tag, float(err[wi]), float(bound[wi]), n=int(err.size))
    if not ok.all():
        b = int(np.argmin(ok))
        fails.append(f"{tag}: {int((~ok).sum())}/{err.size} over the bound (first #{int(idx[b])}: {err[b]:.3e} > {bound[b]:.3e})")


def check_grid(tag, gr: Grid, cells, vm, fails, u=U32, extra_levels=0.0, exact_cells=True):
    """Every node of a read-back grid (cells [M, d], velocity|mass [M, d+1]) against the truth: nodes no particle
    reaches, and nodes of exactly zero truth mass, hold exactly 0. Returns the near-clamp count."""
    d = gr.d
    vm = np.asarray(vm, np.float64)
    assert np.all(np.isfinite(vm)), f"{tag}: non-finite grid values"
    i = gr.lookup(cells)
    if exact_cells:
        assert (i >= 0).sum() == len(gr.keys), f"{tag}: a node some particle reaches is not in the grid"
    zero = (i < 0) | (gr.mass[np.maximum(i, 0)] == 0.0)
    if zero.any():
        nz = np.abs(vm[zero]).max()
        report_margin(f"{tag}: nodes of zero truth mass (max |value|)", float(nz), 0.0, n=int(zero.sum()))
        if nz != 0.0:
            fails.append(f"{tag}: {int((np.abs(vm[zero]).max(1) != 0).sum())} nodes of zero truth mass hold non-zero values")
    j = i[~zero]
    bm, bv, near = gr.bounds(u, extra_levels)
    check(f"{tag}: node mass (scale sum w m, n contributors)", np.abs(vm[~zero, d] - gr.mass[j]), bm[j], fails)
    check(f"{tag}: node velocity (scale sum w |m v + C dpt| / m)", np.linalg.norm(vm[~zero, :d] - gr.vel[j], axis=1), bv[j], fails)
    return int(near[j].sum()), len(j)


def check_particles(tag, pt: Particles, got, model, fails, sel=None, own_F=None):
    """x, v, F and C' of every particle (got: dict or ParticleSet of fp32 outputs in the inputs' order). `own_F` [n] bool: the
    particles whose F is not pt.F by design (projected by the plasticity: tests/plastic_truth.py judges their F); their F
    line is left to the caller, x, v and C' are checked as for every particle."""
    g = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    d = pt.d
    f = lambda k: np.asarray(g(k), np.float64)
    for name, val in (("pos", f("pos")), ("vel", f("vel")), ("def_grad", f("def_grad")), ("affine", f("affine"))):
        assert np.all(np.isfinite(val)), f"{tag}: non-finite {name}"
    check(f"{tag}: x (scale dt |v| + |x|)", np.linalg.norm(f("pos") - pt.x, axis=1), pt.b_x, fails, sel)
    check(f"{tag}: v (scale sum w |v_i|)", np.linalg.norm(f("vel") - pt.vel, axis=1), pt.b_vel, fails, sel)
    sel_F = sel if own_F is None else (~np.asarray(own_F, bool) if sel is None else np.asarray(sel, bool) & ~np.asarray(own_F, bool))
    check(f"{tag}: F (scale dt |grad| |F|)", np.linalg.norm(mat(f("def_grad"), d) - pt.F, axis=(1, 2)), pt.b_F, fails, sel_F)
    Cn, bC = pt.affine(model, f("def_grad"))
    check(f"{tag}: C' (scale m sum w |v_i| |dpt| / h^2 + stress)", np.linalg.norm(mat(f("affine"), d) - Cn, axis=(1, 2)), bC, fails, sel)
    near = pt.near_cap if sel is None else pt.near_cap[sel]
    return int(near.sum())


# ------------------------------------------------------------------------------------------------ scenes
GRAVITY = (1.5, -9.81, 2.5)      # every component non-zero: a kernel that uses g[1] on every axis, or skips one, differs
DT = 1.0e-3
OCCUPANCY = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 31, 32, 33, 63, 64, 65)   # around the rounds of four ranks


def _finish(pos, h, rng, vel=None, uniform=False, model=0, vel_scale=1.0):
    """A ParticleSet at fp32 positions: random v and C' (scaled so that C' dpt is comparable to m v), F near I, elastic
    (phase 1, no fracture), per-particle mass and material unless `uniform` (the library's uniform-material layout)."""
    from wgsparkl_amd.models import ElasticCoefficients, ParticlePhase
    from wgsparkl_amd.solver import ParticleSet, SimulationParams
    pos = np.asarray(pos, np.float32)
    n, d = pos.shape
    ps = ParticleSet.uniform(pos, h / 4.0, 10.0, ElasticCoefficients.from_young_modulus(1e5, 0.3), phase=ParticlePhase(1.0, -1.0))
    ps.vel[:] = (rng.normal(0.0, vel_scale, (n, d)) if vel is None else vel).astype(np.float32)
    ps.affine[:] = (rng.normal(0.0, vel_scale / h, (n, d * d)) * ps.mass[:, None]).astype(np.float32)
    ps.def_grad[:] = (np.eye(d).reshape(-1) + rng.normal(0.0, 0.01, (n, d * d))).astype(np.float32)
    if not uniform:
        for k in ("mass", "init_volume", "lambda_", "mu"):
            v = getattr(ps, k)
            v[:] = (v * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    # enough blocks for the stencils of every particle
    cells = assoc_cell(pos, h)
    blocks = np.unique(np.concatenate([(cells + np.array(s)) // bw_of(d) for s in shifts_of(d) * 2 // 2]), axis=0)
    cap = int(2 ** np.ceil(np.log2(max(64, 2 * len(blocks) + 64))))
    return dict(particles=ps, params=SimulationParams(gravity=GRAVITY[:d], dt=DT), colliders=[], cell_width=float(h),
                grid_capacity=cap, model=model)


def _in_cell(cells, h, rng):
    """fp32 positions whose associated cell (round(x / h) - 1) is `cells` [n, d], away from the ties"""
    x = ((np.asarray(cells, np.float64) + 1.0 + rng.uniform(-0.45, 0.45, np.shape(cells))) * h).astype(np.float32)
    assert np.array_equal(assoc_cell(x, h), cells)
    return x


def source_patterns(d, h, seed=0, **kw):
    """Every non-empty subset of a target block b's 2^d source blocks b - {0,1}^d, each its own island (islands 4 blocks
    apart): every source holds 1-3 particles in cells whose stencils reach b (cells BW-2, BW-1 along an axis where the
    source lies below b). b holds particles only when b itself is in the subset."""
    rng = np.random.default_rng(seed)
    bw = bw_of(d)
    offs = shifts_of(d) % 2
    offs = np.unique(offs, axis=0)                                       # {0,1}^d
    cells = []
    for mask in range(1, 2 ** len(offs)):
        i = mask - 1
        tgt = np.array([4 * (i % 16) + 2, 2, 4 * (i // 16) + 2][:d]) if d == 3 else np.array([4 * i + 2, 2])
        for j, o in enumerate(offs):
            if not mask >> j & 1:
                continue
            src = tgt - o
            for _ in range(int(rng.integers(1, 4))):
                lc = np.where(o == 1, rng.integers(bw - 2, bw, d), rng.integers(0, bw, d))
                cells.append(src * bw + lc)
    cells = np.array(cells)
    return _finish(_in_cell(cells, h, rng), h, rng, **kw)


def occupancy(d, h, seed=1, **kw):
    """Blocks whose occupied cells hold each count of OCCUPANCY particles, next to empty cells."""
    rng = np.random.default_rng(seed)
    bw = bw_of(d)
    cells = []
    for i, k in enumerate(OCCUPANCY):
        blk = np.array([3 * i + 1, 1, 1][:d])
        a = np.array([1, 1, 1][:d]) if d == 3 else np.array([2, 2])
        b = a.copy()
        b[0] += 2                                                        # an empty cell between the two
        cells += [blk * bw + a] * k
        cells += [blk * bw + b] * OCCUPANCY[(i + 7) % len(OCCUPANCY)]
    cells = np.array(cells)
    return _finish(_in_cell(cells, h, rng), h, rng, **kw)


def coordinates(d, h, seed=2, **kw):
    """A cluster straddling 0 on every axis, and clusters two blocks inside every corner of the packed key range
    (3D: x, z in [-1023, 1024] blocks, y in [-511, 512]; 2D: [-32767, 32768])."""
    rng = np.random.default_rng(seed)
    bw = bw_of(d)
    pos = [rng.uniform(-2.0 * h, 2.0 * h, (60, d))]
    edges = [(-1021, 1022), (-509, 510), (-1021, 1022)] if d == 3 else [(-32765, 32766)] * 2
    for corner in np.ndindex(*([2] * d)):
        blk = np.array([edges[k][corner[k]] for k in range(d)])
        cells = blk * bw + rng.integers(0, bw, (20, d))
        pos.append(_in_cell(cells, h, rng).astype(np.float64))
    return _finish(np.concatenate(pos), h, rng, **kw)


def ties(d, h, seed=3, **kw):
    """Positions on the ties x / h = k + 0.5 (power-of-two h: exact, so a weight is exactly 0), or one ulp either side of
    the fp32 (k + 0.5) h (other h: where the division rule and x * (1 / h) may pick different cells)."""
    rng = np.random.default_rng(seed)
    n = 400
    k = rng.integers(-40, 40, (n, d)).astype(np.float64)
    x = ((k + 0.5) * h).astype(np.float32)
    if not _pow2(h):
        x = np.nextafter(x, np.where(rng.random((n, d)) < 0.5, -np.inf, np.inf).astype(np.float32))
    keep = rng.random((n, d)) < 0.6                                      # the other coordinates anywhere
    x = np.where(keep, x, rng.uniform(-40 * h, 40 * h, (n, d))).astype(np.float32)
    return _finish(x, h, rng, **kw)


def clamps(d, h, seed=4, **kw):
    """Velocities whose node values and particle speeds straddle h / dt (C' = 0: the node velocities are the particles')."""
    rng = np.random.default_rng(seed)
    bw = bw_of(d)
    n = 600
    cells = rng.integers(0, 6 * bw, (n, d))
    lim = h / DT
    vel = lim * rng.uniform(-1.4, 1.4, (n, d))
    sc = _finish(_in_cell(cells, h, rng), h, rng, vel=vel, **kw)
    sc["particles"].affine[:] = 0.0
    return sc


def _pow2(h):
    m, _ = np.frexp(h)
    return m == 0.5


def division_rule_differs(pos32, h):
    """positions [n, d] whose fp32 round(x / h) and round(x * fl(1 / h)) differ on some axis"""
    h32 = np.float32(h)
    a = np.rint(pos32 / h32)
    b = np.rint(pos32 * (np.float32(1.0) / h32))
    return np.any(a != b, axis=1)


SCENES = dict(source_patterns=source_patterns, occupancy=occupancy, coordinates=coordinates, ties=ties, clamps=clamps)
