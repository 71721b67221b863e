"""Truth of a simulation with per-particle constitutive models (MpmData.set_particle_models; include/wgsparkl_hip.h): the substep of
oracle/np_oracle.py with the particle update chosen row by row — fluid rows advance J and take the Tait / viscous stress exactly as
tests/fluid_truth.py's FluidState does, solid rows take F <- F + dt G F and oracle/np_oracle.py's kirchoff_stress of the solid's model.
The transfers do not know the model: they are NpState's own, and only the constitutive hook is here. An all-fluid mask reproduces
FluidState array for array, an all-solid one NpState.

TEST INFRASTRUCTURE ONLY. No colliders. float64 is the truth, float32 the error a plain restatement makes in the step's own precision
(helpers.assert_close_to_truth's `ref32`). Also here: the coupled scenes the GPU parity test runs, and their two truths, computed once."""
import functools

import numpy as np

from fluid_truth import FluidState, advance_j, fluid_def_grad, kirchhoff
from oracle.np_oracle import kirchoff_stress, mat, unmat
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

    def _constitutive(self, grad):
        """by the row's own model"""
        d, T, dt = self.d, self.dtype, self.dt_t
        fl, so = self.fluid, ~self.fluid
        tau = np.zeros((len(fl), d, d), T)
        if fl.any():
            J = advance_j(self.J[fl], grad[fl], dt)
            tau[fl] = kirchhoff(J, grad[fl], self.lam[fl], self.mu[fl], self.gamma)
            self.J[fl] = J
            self.F[fl] = fluid_def_grad(J, d)
        if so.any():
            Fm = mat(self.F[so], d)
            Fm = Fm + (grad[so] * dt) @ Fm
            tau[so] = kirchoff_stress(self.solid_model, self.lam[so], self.mu[so], Fm).astype(T)   # (its np.eye is fp64: rounded back once)
            self.F[so] = unmat(Fm)
            self.J[so] = np.linalg.det(Fm).astype(T)
        return tau


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
