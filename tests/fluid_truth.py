"""Truth of the weakly-compressible fluid model (MODEL_FLUID; include/wgsparkl_hip.h): the substep of oracle/np_oracle.py with
the fluid's particle update in place of F / kirchoff_stress, written from the formulae of the header and nothing else.

TEST INFRASTRUCTURE ONLY. No colliders. Takes a dtype: float64 is the truth, float32 the error a plain restatement of the same
formulae makes in the step's own precision (helpers.assert_close_to_truth's `ref32`). Nothing here is tuned for accuracy: the
determinant is that of I + dt G as written, the power is the power."""
import numpy as np

from oracle.np_oracle import NpState, _mat, _unmat, assoc_cell, eval_all

J_MIN = 1.0e-10   # the clamp of neo_hookean_elasticity.wgsl:14-25


def advance_j(J, G, dt):
    """J' = J det(I + dt G). G: [n, r, c] in the arrays' dtype."""
    d = G.shape[1]
    eye = np.eye(d, dtype=G.dtype)
    return J * np.linalg.det(eye + G * G.dtype.type(dt)).astype(G.dtype)


def pressure(J, lam, gamma):
    """Tait: p = lambda / gamma (Jc^-gamma - 1), Jc = max(J, 1e-10)."""
    t = J.dtype.type
    Jc = np.maximum(J, t(J_MIN))
    return lam / t(gamma) * (Jc ** t(-gamma) - t(1.0))


def kirchhoff(J, G, lam, mu, gamma):
    """tau = -Jc p I + Jc mu (G + G^T)   [n, r, c]."""
    t = J.dtype.type
    d = G.shape[1]
    Jc = np.maximum(J, t(J_MIN))
    p = pressure(J, lam, gamma)
    eye = np.eye(d, dtype=J.dtype)
    return (-(Jc * p))[:, None, None] * eye + (Jc * mu)[:, None, None] * (G + G.transpose(0, 2, 1))


def psi_parts(J, lam, gamma):
    """The additive pieces of Psi(Jc) = lambda / gamma (Jc^(1-gamma) / (gamma-1) + Jc - gamma / (gamma-1)) in fp64, arranged as
    lambda / gamma ((Jc^(1-gamma) - 1) / (gamma-1)) and lambda / gamma (Jc - 1): dPsi/dJ = -p, Psi(1) = 0. -> [n, 2]"""
    J = np.asarray(J, np.float64)
    lam = np.asarray(lam, np.float64)
    Jc = np.maximum(J, J_MIN)
    a = lam / gamma * np.expm1((1.0 - gamma) * np.log(Jc)) / (gamma - 1.0)
    b = lam / gamma * (Jc - 1.0)
    return np.stack([a, b], 1)


def psi(J, lam, gamma):
    return psi_parts(J, lam, gamma).sum(1)


def fluid_def_grad(J, d):
    """The canonical def_grad of a fluid particle: diag(J, 1[, 1]), column-major [n, d*d]."""
    F = np.tile(np.eye(d, dtype=J.dtype).reshape(-1), (len(J), 1))
    F[:, 0] = J
    return F


class FluidState(NpState):
    """Particle state + one substep of the fluid in `dtype` (no colliders). `J` replaces F; `F` is kept as diag(J, 1[, 1])."""

    def __init__(self, particles, params, cell_width, gamma=7.0, dtype=np.float64):
        super().__init__(particles, params, cell_width, model=2)
        self.dtype = np.dtype(dtype)
        t = self.dtype.type
        for name in ("pos", "vel", "C", "mass", "vol", "lam", "mu"):
            # (the inputs are fp32 values: exact in either dtype)
            setattr(self, name, getattr(self, name).astype(self.dtype))
        self.J = np.linalg.det(_mat(np.asarray(particles.def_grad, np.float64), self.d)).astype(self.dtype)
        self.F = fluid_def_grad(self.J, self.d)
        self.g = self.g.astype(self.dtype)
        self.gamma = float(gamma)
        self.dt_t, self.h_t = t(self.dt), t(self.h)
        self.cells0 = None

    def _substep(self):
        d, T = self.d, self.dtype
        t = T.type
        h, dt = self.h_t, self.dt_t
        n = self.pos.shape[0]
        cell = assoc_cell(self.pos.astype(np.float32), self.h)           # [n, d] (the bit-exact rule, on the fp32 position)
        self.cells0 = cell
        ref = cell.astype(T) * h - self.pos
        w = eval_all(-ref / h).astype(T)                                  # [n, d, 3]
        shifts = np.stack(np.meshgrid(*([np.arange(3)] * d), indexing="ij"), -1).reshape(-1, d)
        wn = np.ones((n, len(shifts)), T)
        for k in range(d):
            wn *= w[:, k, shifts[:, k]]
        dpt = ref[:, None, :] + shifts[None, :, :].astype(T) * h
        node = cell[:, None, :] + shifts[None, :, :]
        # ---- P2G
        Cm = _mat(self.C, d)
        mom = np.einsum("nrc,nsc->nsr", Cm, dpt) + (self.mass[:, None] * self.vel)[:, None, :]
        lo = node.reshape(-1, d).min(0)
        ext = node.reshape(-1, d).max(0) - lo + 1
        flat = np.ravel_multi_index(tuple((node - lo).reshape(-1, d).T), tuple(ext)).reshape(n, -1)
        gm = np.zeros((int(np.prod(ext)), d), T)
        gmass = np.zeros(int(np.prod(ext)), T)
        np.add.at(gm, flat.reshape(-1), (mom * wn[:, :, None]).reshape(-1, d))
        np.add.at(gmass, flat.reshape(-1), (self.mass[:, None] * wn).reshape(-1))
        # ---- grid update
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.where(gmass > 0, t(1.0) / gmass, t(0.0)).astype(T)
        gv = (gm + gmass[:, None] * self.g[None, :] * dt) * inv[:, None]
        gv = np.clip(gv, -h / dt, h / dt)
        self.grid = dict(lo=lo, ext=ext, vel=gv, mass=gmass)
        # ---- G2P
        nv = gv[flat]
        vel = np.einsum("ns,nsr->nr", wn, nv)
        invd = t(4.0) / (h * h)
        grad = invd * np.einsum("ns,nsr,nsc->nrc", wn, nv, dpt)          # G [n, r, c]
        # ---- particle update, no colliders
        speed = np.linalg.norm(vel, axis=1)
        too_fast = speed > h / dt
        vel[too_fast] = vel[too_fast] / speed[too_fast, None] * h / dt
        self.pos = self.pos + vel * dt
        self.J = advance_j(self.J, grad, dt)
        tau = kirchhoff(self.J, grad, self.lam, self.mu, self.gamma)
        Cn = grad * self.mass[:, None, None] - tau * (self.vol * invd * dt)[:, None, None]
        assert vel.dtype == T and Cn.dtype == T and self.J.dtype == T and self.pos.dtype == T
        self.vel = vel
        self.F = fluid_def_grad(self.J, d)
        self.C = _unmat(Cn)
        self.last_grad = grad

    # -- what the GPU read-backs are compared with
    def active_blocks(self):
        """Virtual ids of the blocks active in the last substep (grid.wgsl:300-320: the block of every particle's associated cell
        and its "+" neighbours), sorted lexicographically, and the particle count of each."""
        bw = 4 if self.d == 3 else 8
        b = np.floor_divide(self.cells0, bw)
        own, cnt = np.unique(b, axis=0, return_counts=True)
        offs = np.stack(np.meshgrid(*([np.arange(2)] * self.d), indexing="ij"), -1).reshape(-1, self.d)
        allb = np.unique((own[:, None, :] + offs[None, :, :]).reshape(-1, self.d), axis=0)
        allb = allb[np.lexsort(allb.T[::-1])]
        counts = {tuple(k): int(c) for k, c in zip(own.tolist(), cnt.tolist())}
        return allb, np.array([counts.get(tuple(k), 0) for k in allb.tolist()], np.uint32)

    def grid_records(self):
        """(cells, velocity|mass) of every node of the active blocks, sorted by cell like MpmData.read_grid."""
        bw = 4 if self.d == 3 else 8
        blocks, _ = self.active_blocks()
        loc = np.stack(np.meshgrid(*([np.arange(bw)] * self.d), indexing="ij"), -1).reshape(-1, self.d)
        cells = (blocks[:, None, :] * bw + loc[None, :, :]).reshape(-1, self.d)
        cells = cells[np.lexsort(cells.T[::-1])]
        v, m = self.grid_at(cells)
        return cells.astype(np.int32), np.concatenate([v, m[:, None]], 1)

    def kinetic(self):
        return float(0.5 * np.sum(np.asarray(self.mass, np.float64) * np.sum(np.asarray(self.vel, np.float64) ** 2, 1)))

    def momentum(self):
        return np.sum(np.asarray(self.mass, np.float64)[:, None] * np.asarray(self.vel, np.float64), 0)
