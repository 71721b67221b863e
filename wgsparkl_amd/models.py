"""Material models — host-side mirror of the reference's `wgsparkl::models`.

Reference: src/models/mod.rs:52-75 (ElasticCoefficients, lame_lambda_mu),
src/models/drucker_prager.rs:6-53 (DruckerPrager, DruckerPragerPlasticState).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

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


# Force fields (include/wgsparkl_hip_forces.h WGS_FORCE_* / WGS_REGION_*; no reference counterpart: the reference's only body force is
# the gravity of its SimulationParams)
FORCE_NONE = 0
FORCE_UNIFORM = 1    # v += dt * vec
FORCE_RADIAL = 2     # toward `center` (strength > 0 attracts)
FORCE_VORTEX = 3     # about the axis `vec` through `center` (2D: +z)
FORCE_DRAG = 4       # backward Euler relaxation toward the velocity `vec` at the rate `strength`
REGION_ALL = 0
REGION_BOX = 1       # |x_k - region_center_k| <= region_half_k on every axis
REGION_BALL = 2      # |x - region_center|^2 <= region_half[0]^2
MAX_FORCE_FIELDS = 8


def _vec3(v):
    v = tuple(float(x) for x in v)
    if not 1 <= len(v) <= 3:
        raise ValueError("a vector of a force field has 2 or 3 components")
    return v + (0.0,) * (3 - len(v))


@dataclass(frozen=True)
class ForceField:
    """One entry of `MpmData.set_force_fields`: a rule on the grid nodes' velocities (the header's "The rule"), applied once per substep
    behind the grid update and in front of the domain walls, to the nodes with mass inside its region. Made by `uniform`, `radial`,
    `vortex` or `drag`; `.within_box` / `.within_ball` give the same field confined to a region. Vectors take 2 or 3 components (the
    third is ignored in 2D). A region face meant to lie between two nodes goes at (k + 1/2) h."""
    kind: int = FORCE_NONE
    falloff: int = 0
    region: int = REGION_ALL
    strength: float = 0.0
    softening: float = 0.0
    center: tuple = (0.0, 0.0, 0.0)
    vec: tuple = (0.0, 0.0, 0.0)
    region_center: tuple = (0.0, 0.0, 0.0)
    region_half: tuple = (0.0, 0.0, 0.0)

    @staticmethod
    def uniform(acceleration) -> "ForceField":
        """v += dt * acceleration"""
        return ForceField(FORCE_UNIFORM, vec=_vec3(acceleration))

    @staticmethod
    def radial(center, strength: float, falloff: int = 0, softening: float = 0.0) -> "ForceField":
        """r = center - x, q = |r|^2 + softening^2: v += dt * strength * w_falloff(q) * r — strength > 0 attracts; falloff 0: a spring
        toward the centre, 3: an inverse-square attraction"""
        return ForceField(FORCE_RADIAL, int(falloff), strength=float(strength), softening=float(softening), center=_vec3(center))

    @staticmethod
    def vortex(center, strength: float, axis=(0.0, 0.0, 1.0), falloff: int = 0, softening: float = 0.0) -> "ForceField":
        """a swirl about the line through `center` along `axis` (2D: about +z); falloff 0: a rigid spin-up, 2: a line vortex"""
        return ForceField(FORCE_VORTEX, int(falloff), strength=float(strength), softening=float(softening), center=_vec3(center), vec=_vec3(axis))

    @staticmethod
    def drag(rate: float, toward=(0.0, 0.0, 0.0)) -> "ForceField":
        """relaxation toward the velocity `toward` at `rate` per second (backward Euler: stable for any rate; a huge rate prescribes it)"""
        return ForceField(FORCE_DRAG, strength=float(rate), vec=_vec3(toward))

    def within_box(self, center, half) -> "ForceField":
        return replace(self, region=REGION_BOX, region_center=_vec3(center), region_half=_vec3(half))

    def within_ball(self, center, radius: float) -> "ForceField":
        return replace(self, region=REGION_BALL, region_center=_vec3(center), region_half=(float(radius), 0.0, 0.0))


# Particles added at run time (include/wgsparkl_hip_emit.h; no reference counterpart: the reference's MpmData holds what it was created with)
MAX_EMITTERS = 8


@dataclass(frozen=True)
class Emitter:
    """One entry of `MpmData.set_emitters`: an axis-aligned lattice box of prod(count) particles, emitted again every `period` substeps
    (the header's "Schedule" and "Positions"). `proto`: a `ParticleSet` of ONE particle — everything but its position is copied, its
    velocity is the emission velocity; `model`: the MODEL_* of the emitted particles, read only while the data carries a per-particle
    table. Point (i_0, ..) of a batch sits at lo_k + (i_k + 1/2) spacing + jitter * spacing * u_k, u_k in [-1/2, 1/2) from the hash of
    (seed, emitter index, batch number, point index, axis). `batches` = 0: no limit. A batch that does not fit whole into the remaining
    particle capacity is skipped and counted (`MpmData.emitter_counts`)."""
    proto: object
    lo: tuple
    count: tuple
    spacing: float
    model: int = MODEL_COROTATED
    jitter: float = 0.0
    seed: int = 0
    start_substep: int = 0
    period: int = 1
    batches: int = 0

    def __post_init__(self):
        dim = int(self.proto.dim)
        if self.proto.n != 1:
            raise ValueError("Emitter: proto is a ParticleSet of exactly one particle")
        if len(self.lo) != dim or len(self.count) != dim:
            raise ValueError("Emitter: lo and count have one entry per axis of the proto")
        if any(int(c) != c or int(c) < 1 for c in self.count):
            raise ValueError("Emitter: every count is an integer >= 1")
        if int(self.period) != self.period or int(self.period) < 1:
            raise ValueError("Emitter: period is an integer >= 1")
        if not (math.isfinite(self.jitter) and 0.0 <= self.jitter <= 0.5):
            raise ValueError("Emitter: jitter in [0, 0.5] (a fraction of the spacing)")
        if not math.isfinite(self.spacing):
            raise ValueError("Emitter: spacing finite")
        if int(self.model) not in (MODEL_COROTATED, MODEL_NEO_HOOKEAN, MODEL_FLUID):
            raise ValueError("Emitter: model is a MODEL_* value")
        for name in ("seed", "start_substep", "batches"):
            v = getattr(self, name)
            if int(v) != v or not 0 <= int(v) < 2 ** 32:
                raise ValueError(f"Emitter: {name} is an unsigned 32-bit integer")

    @property
    def batch_size(self) -> int:
        return int(np.prod([int(c) for c in self.count], dtype=np.int64))

    @staticmethod
    def nozzle(proto, lo, count, spacing: float, dt: float, thickness: float = None, **kw) -> "Emitter":
        """An emitter whose batches follow each other without a gap or an overlap: a slab of `thickness` (default: the lattice's extent
        along the largest component of the emission velocity) leaves the nozzle every period = ceil(thickness / (|v| dt)) substeps."""
        v = np.asarray(proto.vel[0], np.float64)
        speed = float(np.linalg.norm(v))
        if not speed > 0.0 or not dt > 0.0:
            raise ValueError("Emitter.nozzle: the proto needs a velocity and dt must be > 0")
        if thickness is None:
            thickness = int(count[int(np.argmax(np.abs(v)))]) * float(spacing)
        period = max(1, int(math.ceil(float(thickness) / (speed * float(dt)) - 1e-9)))
        return Emitter(proto, tuple(float(x) for x in lo), tuple(int(c) for c in count), float(spacing), period=period, **kw)


# Particles removed at run time (include/wgsparkl_hip_remove.h WGS_SINK_*; no reference counterpart, like the emitters)
SINK_INSIDE = 0      # removes the particles inside the region
SINK_OUTSIDE = 1     # removes the particles that are NOT inside it: an outflow boundary (takes a particle with a NaN position)
MAX_SINKS = 8


@dataclass(frozen=True)
class Sink:
    """One entry of `MpmData.set_sinks` / `MpmData.remove_particles_in`: a region (`REGION_BOX`: |x_k - center_k| <= half_k on every
    axis, `REGION_BALL`: |x - center|^2 <= half[0]^2, both in fp32 from the stored position, a face counting as inside), the `side` it
    removes, and — read by `set_sinks` only — the schedule: due in front of substep s if s >= start_substep and (s - start_substep) %
    period == 0. Vectors take 2 or 3 components (the third is ignored in 2D). Made by `box`, `ball` or `outside_box`."""
    region: int = REGION_BOX
    side: int = SINK_INSIDE
    center: tuple = (0.0, 0.0, 0.0)
    half: tuple = (0.0, 0.0, 0.0)
    start_substep: int = 0
    period: int = 1

    def __post_init__(self):
        if int(self.region) not in (REGION_BOX, REGION_BALL):
            raise ValueError("Sink: region is REGION_BOX or REGION_BALL")
        if int(self.side) not in (SINK_INSIDE, SINK_OUTSIDE):
            raise ValueError("Sink: side is SINK_INSIDE or SINK_OUTSIDE")
        if len(self.center) != 3 or len(self.half) != 3:
            raise ValueError("Sink: center and half have three components (Sink.box / Sink.ball pad them)")
        if not all(math.isfinite(x) for x in self.center):
            raise ValueError("Sink: center finite")
        if not all(math.isfinite(x) and x >= 0.0 for x in self.half):
            raise ValueError("Sink: half finite and >= 0")
        if int(self.period) != self.period or not 1 <= int(self.period) < 2 ** 32:
            raise ValueError("Sink: period is an integer >= 1")
        if int(self.start_substep) != self.start_substep or not 0 <= int(self.start_substep) < 2 ** 32:
            raise ValueError("Sink: start_substep is an unsigned 32-bit integer")

    @staticmethod
    def box(center, half, **kw) -> "Sink":
        """removes what is inside the axis-aligned box"""
        return Sink(REGION_BOX, SINK_INSIDE, _vec3(center), _vec3(half), **kw)

    @staticmethod
    def ball(center, radius: float, **kw) -> "Sink":
        """removes what is inside the ball (a disc in 2D)"""
        return Sink(REGION_BALL, SINK_INSIDE, _vec3(center), (float(radius), 0.0, 0.0), **kw)

    @staticmethod
    def outside_box(center, half, **kw) -> "Sink":
        """removes what is NOT inside the box: everything that leaves it"""
        return Sink(REGION_BOX, SINK_OUTSIDE, _vec3(center), _vec3(half), **kw)
