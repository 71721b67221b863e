"""Material models — host-side mirror of the reference's `wgsparkl::models`.

Reference: src/models/mod.rs:52-75 (ElasticCoefficients, lame_lambda_mu),
src/models/drucker_prager.rs:6-53 (DruckerPrager, DruckerPragerPlasticState).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

F32 = np.float32

# Constitutive model ids (the reference selects at shader-compile time,
# src/solver/particle_update.wgsl:7-8; here it is a runtime per-MpmData choice).
MODEL_COROTATED = 0      # models/linear_elasticity.wgsl (reference default)
MODEL_NEO_HOOKEAN = 1    # models/neo_hookean_elasticity.wgsl
MODEL_PER_PARTICLE = 3   # what the diagnostics report while a per-particle table is set (MpmData.set_particle_models); never a model to select
MODEL_FLUID = 2          # weakly-compressible Tait fluid + viscosity (no reference counterpart; include/wgsparkl_hip.h WGS_MODEL_FLUID)


def lame_lambda_mu(young_modulus: float, poisson_ratio: float):
    """src/models/mod.rs:52-63, evaluated in f32 like the Rust code."""
    e = F32(young_modulus)
    nu = F32(poisson_ratio)
    one = F32(1.0)
    two = F32(2.0)
    lam = e * nu / ((one + nu) * (one - two * nu))
    mu = e / (two * (one + nu))
    return F32(lam), F32(mu)


@dataclass(frozen=True)
class ElasticCoefficients:
    """src/models/mod.rs:65-75"""
    lambda_: float
    mu: float

    @staticmethod
    def from_young_modulus(young_modulus: float, poisson_ratio: float) -> "ElasticCoefficients":
        lam, mu = lame_lambda_mu(young_modulus, poisson_ratio)
        return ElasticCoefficients(float(lam), float(mu))


@dataclass(frozen=True)
class FluidCoefficients:
    """Material of MODEL_FLUID: the two slots of ElasticCoefficients reinterpreted — `lambda_` carries the bulk modulus at rest,
    `mu` the dynamic viscosity (include/wgsparkl_hip.h WGS_MODEL_FLUID). Usable wherever ElasticCoefficients is."""
    bulk_modulus: float
    viscosity: float = 0.0

    @property
    def lambda_(self) -> float:
        return float(self.bulk_modulus)

    @property
    def mu(self) -> float:
        return float(self.viscosity)

    def arrays(self, n: int):
        """(lambda_, mu) as float32 arrays of n particles."""
        return np.full(n, self.bulk_modulus, F32), np.full(n, self.viscosity, F32)


@dataclass(frozen=True)
class DruckerPrager:
    """src/models/drucker_prager.rs:6-34"""
    h0: float
    h1: float
    h2: float
    h3: float
    lambda_: float
    mu: float

    @staticmethod
    def new(young_modulus: float, poisson_ratio: float) -> "DruckerPrager":
        if young_modulus > 0.0:
            lam, mu = lame_lambda_mu(young_modulus, poisson_ratio)
        else:
            lam, mu = F32(-1.0), F32(-1.0)
        rad = lambda deg: float(F32(deg) * F32(math.pi) / F32(180.0))
        return DruckerPrager(rad(35.0), rad(9.0), 0.2, rad(10.0), float(lam), float(mu))

    def as_array(self):
        return np.array([self.h0, self.h1, self.h2, self.h3, self.lambda_, self.mu], dtype=F32)


# Plasticity rule of an MpmData (include/wgsparkl_hip.h WGS_PLASTICITY_*; `MpmData.set_plasticity_model`): what the six plasticity
# slots of a particle mean and which projection the plastic particle update applies.
PLASTICITY_DRUCKER_PRAGER = 0   # models/drucker_prager.wgsl (reference default)
PLASTICITY_SNOW = 1             # singular-value clamp with hardening (Stomakhin et al. 2013; no reference counterpart)


@dataclass(frozen=True)
class Snow:
    """Parameters of PLASTICITY_SNOW, carried in the six slots of `DruckerPrager` reinterpreted (include/wgsparkl_hip.h
    "Snow plasticity"): h0 = theta_c (critical compression), h1 = theta_s (critical stretch), h2 = xi (hardening coefficient),
    h3 = the cap on the hardening exponent xi (1 - Jp), lambda = the switch (non-zero: on), mu unused. The elastic lambda, mu of
    the particle are its ElasticCoefficients. Usable wherever a DruckerPrager is (`ParticleSet.uniform(plasticity=Snow())`).
    Preconditions (checked here, documented in the header): 0 <= theta_c < 1, theta_s >= 0, xi and max_exponent finite."""
    theta_c: float = 2.5e-2
    theta_s: float = 7.5e-3
    xi: float = 10.0
    max_exponent: float = 5.0

    def __post_init__(self):
        if not (math.isfinite(self.theta_c) and 0.0 <= self.theta_c < 1.0):
            raise ValueError("Snow: 0 <= theta_c < 1")
        if not (math.isfinite(self.theta_s) and self.theta_s >= 0.0):
            raise ValueError("Snow: theta_s >= 0 and finite")
        if not (math.isfinite(self.xi) and math.isfinite(self.max_exponent)):
            raise ValueError("Snow: xi and max_exponent finite")
        # (the kernel reads the fp32 values: theta_c must still be below 1 there)
        if not float(F32(self.theta_c)) < 1.0:
            raise ValueError("Snow: theta_c rounds to 1 in fp32")

    # the slots under their DruckerPrager names: whatever packs a DruckerPrager packs a Snow
    h0 = property(lambda self: float(self.theta_c))
    h1 = property(lambda self: float(self.theta_s))
    h2 = property(lambda self: float(self.xi))
    h3 = property(lambda self: float(self.max_exponent))
    lambda_ = property(lambda self: 1.0)
    mu = property(lambda self: 0.0)

    def as_array(self):
        return np.array([self.theta_c, self.theta_s, self.xi, self.max_exponent, 1.0, 0.0], dtype=F32)


# src/models/drucker_prager.rs:44-53
DRUCKER_PRAGER_DEFAULT_STATE = np.array([1.0, 1.0, 0.0], dtype=F32)


@dataclass(frozen=True)
class ParticlePhase:
    """src/solver/particle_update.rs:35-40"""
    phase: float
    max_stretch: float


# Domain walls (include/wgsparkl_hip.h WGS_WALL_*; no reference counterpart: the reference builds its containers from collider cuboids)
WALL_NONE = 0
WALL_STICKY = 1      # v = 0
WALL_SLIP = 2        # normal component 0, Coulomb friction on the rest
WALL_SEPARATE = 3    # like WALL_SLIP for nodes moving into the wall, free otherwise


@dataclass(frozen=True)
class Wall:
    """One face of `MpmData.set_domain_walls`: a half-space of grid nodes, `cell[k] <= plane` (a low face) or `cell[k] >= plane` (a high
    face) — which axis and which side is the entry's place in the list (2 * k: low face of axis k, 2 * k + 1: its high face). Material comes
    to rest on the inner side of the plane (the lowest particles 0.1 to 0.5 cells inside it), so the plane goes on the surface wanted; no
    particle ever gets further than 1.5 cells beyond it."""
    type: int = WALL_SLIP
    friction: float = 0.0
    plane: int = 0

    @staticmethod
    def low(coordinate: float, h: float, type: int = WALL_SLIP, friction: float = 0.0) -> "Wall":
        """The low face whose last node is the one at or below world coordinate `coordinate`: plane = floor(coordinate / h)."""
        return Wall(int(type), float(friction), int(math.floor(coordinate / h)))

    @staticmethod
    def high(coordinate: float, h: float, type: int = WALL_SLIP, friction: float = 0.0) -> "Wall":
        """The high face whose first node is the one at or above `coordinate`: plane = ceil(coordinate / h)."""
        return Wall(int(type), float(friction), int(math.ceil(coordinate / h)))
