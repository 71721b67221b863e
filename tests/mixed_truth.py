"""Truth of a simulation with per-particle constitutive models (MpmData.set_particle_models; include/wgsparkl_hip.h): the substep of
tests/fluid_truth.py with the particle update chosen row by row — fluid rows advance J and take the Tait / viscous stress exactly as
FluidState does, solid rows take F <- F + dt G F and oracle/np_oracle.py's kirchoff_stress of the solid's model. The transfers do not
know the model, so everything else is FluidState's, statement for statement: an all-fluid mask reproduces it array for array.

TEST INFRASTRUCTURE ONLY. No colliders. float64 is the truth, float32 the error a plain restatement makes in the step's own precision
(helpers.assert_close_to_truth's `ref32`). Also here: the coupled scenes the GPU parity test runs, and their two truths, computed once."""
import functools

import numpy as np

from fluid_truth import FluidState, advance_j, fluid_def_grad, kirchhoff
from oracle.np_oracle import _mat, _unmat, assoc_cell, eval_all, kirchoff_stress
from wgsparkl_amd import scenes
from wgsparkl_amd.models import MODEL_FLUID, ElasticCoefficients, ParticlePhase
from wgsparkl_amd.solver import ParticleSet, SimulationParams


class MixedState(FluidState):
    """`fluid`: boolean mask of the fluid rows; the other rows are solids of `solid_model` (0 corotated, 1 neo-Hookean). `F` holds
    diag(J, 1[, 1]) on fluid rows and the deformation gradient on solid rows; `J` is meaningful on fluid rows."""

    def __init__(self, particles, params, cell_width, fluid, solid_model, gamma=7.0, dtype=np.float64):
        super().__init__(particles, params, cell_width, gamma, dtype)
        self.fluid = np.asarray(fluid, bool).copy()
        assert self.fluid.shape == (particles.n,)
        self.solid_model = int(solid_model)
        solid = ~self.fluid
        self.F[solid] = np.asarray(particles.def_grad, self.dtype)[solid]     # (fp32 inputs: exact in either dtype)

    def models(self):
        """The table MpmData.set_particle_models takes."""
        return np.where(self.fluid, MODEL_FLUID, self.solid_model).astype(np.uint8)

    def _substep(self):
        d, T = self.d, self.dtype
        t = T.type
        h, dt = self.h_t, self.dt_t
        n = self.pos.shape[0]
        cell = assoc_cell(self.pos.astype(np.float32), self.h)
        self.cells0 = cell
        ref = cell.astype(T) * h - self.pos
        w = eval_all(-ref / h).astype(T)
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
        grad = invd * np.einsum("ns,nsr,nsc->nrc", wn, nv, dpt)
        # ---- particle update, no colliders: by the row's own model
        speed = np.linalg.norm(vel, axis=1)
        too_fast = speed > h / dt
        vel[too_fast] = vel[too_fast] / speed[too_fast, None] * h / dt
        self.pos = self.pos + vel * dt
        fl, so = self.fluid, ~self.fluid
        tau = np.zeros((n, d, d), T)
        F = self.F.copy()
        if fl.any():
            J = advance_j(self.J[fl], grad[fl], dt)
            tau[fl] = kirchhoff(J, grad[fl], self.lam[fl], self.mu[fl], self.gamma)
            self.J[fl] = J
            F[fl] = fluid_def_grad(J, d)
        if so.any():
            Fm = _mat(self.F[so], d)
            Fm = Fm + (grad[so] * dt) @ Fm
            tau[so] = kirchoff_stress(self.solid_model, self.lam[so], self.mu[so], Fm).astype(T)   # (its np.eye is fp64: rounded back once)
            F[so] = _unmat(Fm)
            self.J[so] = np.linalg.det(Fm).astype(T)
        Cn = grad * self.mass[:, None, None] - tau * (self.vol * invd * dt)[:, None, None]
        assert vel.dtype == T and Cn.dtype == T and F.dtype == T and self.pos.dtype == T
        self.vel = vel
        self.F = F
        self.C = _unmat(Cn)
        self.last_grad = grad


# ------------------------------------------------------------------------------------------------ the coupled scenes
SUBSTEPS = 24
PATTERNS = ("plane", "random")


def coupled_scene(dim, solid_model, pattern, gravity=True, seed=4):
    """A jittered block in free fall, part Tait fluid and part elastic solid, whose initial velocity field compresses and shears it: the
    two materials interact through every grid node they share. `plane`: fluid below x = 12.3 (2D: 18.3) — neither a block nor a cell
    boundary, some 40 % of the body —, solid above; `random`: an independent coin per particle (p = 1/2), so that every wave holds both kinds in arbitrary lanes.
    Returns the scene dict; scene["models"] is the table, scene["fluid"] the mask."""
    h = 1.0
    counts = (16, 16, 16) if dim == 3 else (40, 40)
    pos = scenes.lattice(counts, (9.0,) * dim, h, 0.05, seed=seed)
    solid = ElasticCoefficients.from_young_modulus(2.0e5, 0.3)
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, solid, phase=ParticlePhase(1.0, scenes.FLT_MAX))   # (no plastic state)
    if pattern == "plane":
        fluid = pos[:, 0] < (12.3 if dim == 3 else 18.3)
    else:
        fluid = np.random.default_rng(77 + dim).random(ps.n) < 0.5
    ps.lambda_[fluid] = np.float32(2.0e5)      # bulk modulus
    ps.mu[fluid] = np.float32(10.0)            # viscosity
    c = pos.mean(0)
    ps.vel[:] = ((c - pos) * 2.5).astype(np.float32)                   # converging
    ps.vel[:, 0] += ((pos[:, 1] - c[1]) * 3.0).astype(np.float32)      # shear
    g = (0.0, -9.81, 0.0)[:dim] if gravity else (0.0,) * dim
    models = np.where(fluid, MODEL_FLUID, solid_model).astype(np.uint8)
    return dict(particles=ps, params=SimulationParams(gravity=g, dt=1.0 / 1200.0), colliders=[], cell_width=h, grid_capacity=4096,
                model=solid_model, fluid_gamma=7.0, models=models, fluid=fluid)


@functools.lru_cache(maxsize=None)
def coupled_truths(dim, solid_model, pattern):
    """(scene, fp64 state, fp32 state) after SUBSTEPS substeps: computed once, shared by the CPU and the GPU tests, left unchanged."""
    sc = coupled_scene(dim, solid_model, pattern)
    out = [sc]
    for dtype in (np.float64, np.float32):
        st = MixedState(sc["particles"], sc["params"], sc["cell_width"], sc["fluid"], solid_model, sc["fluid_gamma"], dtype)
        st.step(SUBSTEPS)
        out.append(st)
    return tuple(out)
