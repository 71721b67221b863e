"""Truth of the weakly-compressible fluid model (MODEL_FLUID; include/wgsparkl_hip.h): the substep of oracle/np_oracle.py with
the fluid's particle update as its constitutive hook, written from the formulae of the header and nothing else. The transfers are
NpState's own: nothing of them is restated here.

TEST INFRASTRUCTURE ONLY. No colliders. Takes a dtype: float64 is the truth, float32 the error a plain restatement of the same
formulae makes in the step's own precision (helpers.assert_close_to_truth's `ref32`). Nothing here is tuned for accuracy: the
determinant is that of I + dt G as written, the power is the power."""
import numpy as np

from oracle.np_oracle import NpState, mat as _mat

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
        super().__init__(particles, params, cell_width, model=2, dtype=dtype)
        self.J = np.linalg.det(_mat(particles.def_grad, self.d, np.float64)).astype(self.dtype)
        self.F = fluid_def_grad(self.J, self.d)
        self.gamma = float(gamma)

    def _constitutive(self, grad):
        self.J = advance_j(self.J, grad, self.dt_t)
        assert self.J.dtype == self.dtype
        self.F = fluid_def_grad(self.J, self.d)
        return kirchhoff(self.J, grad, self.lam, self.mu, self.gamma)
