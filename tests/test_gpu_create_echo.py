"""-m gpu: what wgs_data_create uploads is what the caller gave it. `MpmData.new` followed by `read_particles()` with no step in
between returns every field of the input bit for bit, in each layout the creation can choose (general, uniform material, the
three modes of the Drucker-Prager parameters; both dimensions) and at particle counts that leave the padded planes a tail; the
particle ids on the device are the caller's indices; and two slabs of a sharded scene export the state and ids they were given."""
import ctypes as C

import numpy as np
import pytest

from wgsparkl_amd import MpmData, scenes
from wgsparkl_amd.models import DruckerPrager, ParticlePhase
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import SimulationParams

from helpers import pipeline
from gpu_common import export_state_and_cdf

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 130)      # one slot; one short of a 64-slot row; two rows and two slots (npad = 64, 64, 192)
FIELDS = ("pos", "vel", "def_grad", "affine", "cdf_normal", "cdf_rigid_vel", "cdf_dist", "cdf_affinity", "init_volume", "init_radius",
          "mass", "lambda_", "mu", "dp", "phase", "dp_state", "has_plasticity", "has_phase")
# What a particle without Drucker-Prager parameters stands for: DruckerPrager::new(-1, -1) (models/mod.rs:24), the angles in
# fp32 as `degrees * (pi / 180)` — f32::to_radians, and the library's order of evaluation (the last bit depends on it).
_DEG = np.float32(np.float32(np.pi) / np.float32(180.0))
DEFAULT_DP = np.array([np.float32(35.0) * _DEG, np.float32(9.0) * _DEG, 0.2, np.float32(10.0) * _DEG, -1.0, -1.0], np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _random_fields(ps, rng):
    """every field the caller may set, each particle its own values (the cdf too: before any step it is echoed)"""
    n, d = ps.n, ps.dim
    f = lambda *shape: rng.normal(0.0, 1.0, size=shape).astype(np.float32)
    ps.cdf_normal[:] = f(n, d)
    ps.cdf_rigid_vel[:] = f(n, d)
    ps.cdf_dist[:] = f(n)
    ps.cdf_affinity[:] = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    ps.init_radius[:] = rng.uniform(0.1, 0.4, n).astype(np.float32)
    ps.init_volume[:] = rng.uniform(0.01, 0.1, n).astype(np.float32)
    ps.lambda_[:] = rng.uniform(1e4, 1e5, n).astype(np.float32)
    ps.mu[:] = rng.uniform(1e4, 1e5, n).astype(np.float32)
    return ps


def _dp_rows(rng, n, h_per_particle, lame_per_particle):
    one = rng.uniform(0.1, 0.9, 6).astype(np.float32)
    dp = np.tile(one, (n, 1))
    if h_per_particle:
        dp[:, :4] = rng.uniform(0.1, 0.9, (n, 4)).astype(np.float32)
    if lame_per_particle:
        dp[:, 4:] = rng.uniform(1e4, 1e5, (n, 2)).astype(np.float32)
    return dp


def _elastic(n, dim, rng, one_material):
    """no particle ever reaches the plasticity branch: those with a phase carry phase 1 and no stretch limit, those without one
    carry Drucker-Prager parameters whose lambda is 0 — so both flags take both values"""
    ps = _random_fields(scenes.random_cloud(n, dim=dim, seed=int(rng.integers(1 << 30)), phase=ParticlePhase(1.0, -1.0)), rng)
    if one_material:
        for a in (ps.mass, ps.init_volume, ps.lambda_, ps.mu):
            a[:] = a[0]
    elif n > 1:
        ps.lambda_[::2], ps.mu[::2] = ps.lambda_[0], ps.mu[0]          # two materials, interleaved
        ps.lambda_[1::2], ps.mu[1::2] = ps.lambda_[1], ps.mu[1]
    ps.has_phase[:] = rng.random(n) < 0.6
    ps.phase[~ps.has_phase] = (0.0, -1.0)                               # (what has_phase = 0 stands for: models/mod.rs:33-36)
    ps.has_plasticity[:] = ~ps.has_phase | (rng.random(n) < 0.5)
    ps.dp[:] = _dp_rows(rng, n, True, True)
    ps.dp[~ps.has_phase, 4] = 0.0
    ps.dp[~ps.has_plasticity] = DEFAULT_DP
    return ps


def _plastic(n, dim, rng, h_per_particle, lame_per_particle, phases=False):
    """every particle carries Drucker-Prager parameters and reaches the plasticity branch (phase 0, lambda != 0)"""
    ps = _random_fields(scenes.random_cloud(n, dim=dim, seed=int(rng.integers(1 << 30)), plasticity=DruckerPrager.new(1e6, 0.25)), rng)
    ps.dp[:] = _dp_rows(rng, n, h_per_particle, lame_per_particle)
    if phases:                                                           # some with a phase and a stretch limit of their own
        ps.has_phase[:] = rng.random(n) < 0.5
        k = int(ps.has_phase.sum())
        ps.phase[ps.has_phase] = np.stack([rng.integers(0, 2, k), rng.uniform(1.1, 3.0, k)], 1).astype(np.float32)
    return ps


def _layout_of(ps):
    """(plastic, uni_dp, uniform material) as the creation's detections decide them (capi_lifecycle.inc), from the input alone"""
    same = lambda a: bool((_bits(a) == _bits(a)[0]).all())
    ph, ms = ps.phase[:, 0], ps.phase[:, 1]
    plastic = bool((((ph == 0) & (ps.dp[:, 4] != 0)) | ((ph > 0) & (ms > 0) & (ms < np.finfo(np.float32).max))).any())
    uni_dp = 0 if not (plastic and same(ps.dp[:, :4])) else 2 if same(ps.dp[:, 4:]) and same(ms) else 1
    return plastic, uni_dp, ps.dim == 3 and all(same(a) for a in (ps.mass, ps.init_volume, ps.lambda_, ps.mu))


# name -> (the particles, the layout they are built to reach where n > 1: one particle is uniform in every respect)
CASES = {
    "3d two materials (general layout)": (lambda n, rng: _elastic(n, 3, rng, False), (False, 0, False)),
    "3d one material (uniform-material mode)": (lambda n, rng: _elastic(n, 3, rng, True), (False, 0, True)),
    "3d plastic, h0..h3 per particle (uni_dp 0)": (lambda n, rng: _plastic(n, 3, rng, True, True, phases=True), (True, 0, False)),
    "3d plastic, one h0..h3, lambda / mu differ (uni_dp 1)": (lambda n, rng: _plastic(n, 3, rng, False, True), (True, 1, False)),
    "3d plastic, all six equal (uni_dp 2)": (lambda n, rng: _plastic(n, 3, rng, False, False), (True, 2, False)),
    "2d general": (lambda n, rng: _elastic(n, 2, rng, False), (False, 0, False)),
    "2d plastic": (lambda n, rng: _plastic(n, 2, rng, True, True, phases=True), (True, 0, False)),
}


def _device_words(ptr, count, device):
    """`count` 32-bit words at a device address, through a torch tensor of that device"""
    import torch
    t = torch.empty(count, dtype=torch.int32, device=torch.device("cuda", device))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(t.data_ptr(), ptr, 4 * count, 3) == 0          # hipMemcpyDeviceToDevice
    torch.cuda.synchronize(t.device)
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", list(CASES))
def test_create_then_read_echoes_every_field(hip_libs, case, n):
    rng = np.random.default_rng(sorted(CASES).index(case) * 1000 + n)
    make, layout = CASES[case]
    ps = make(n, rng)
    if n > 1:
        assert _layout_of(ps) == layout, "the input does not reach the layout the case is named after"
    given = ps.copy()
    pipe = pipeline(ps.dim)
    params = SimulationParams(gravity=(0.0, -9.81, 0.0)[:ps.dim], dt=1e-3)
    data = MpmData.new(pipe, params, ps, [], 1.0, 1024)
    got = data.read_particles()
    for f in FIELDS:
        assert np.array_equal(_bits(getattr(got, f)), _bits(getattr(given, f))), (case, n, f)
    assert np.array_equal(got.dp_state, np.tile(np.array([1, 1, 0], np.float32), (n, 1)))
    view = data.device_ptrs()
    assert view.count == n and view.capacity == (n + 63) // 64 * 64 and view.dim == ps.dim
    assert np.array_equal(_device_words(view.particle_ids, n, pipe.device), np.arange(n, dtype=np.uint32)), (case, n, "particle ids")
    data.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_two_slabs_export_the_state_and_ids_they_were_given(hip_libs, dim):
    rng = np.random.default_rng(40 + dim)
    ps = _random_fields(scenes.random_cloud(300, dim=dim, seed=50 + dim, phase=ParticlePhase(1.0, -1.0)), rng)
    given = ps.copy()
    sc = dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0)[:dim], dt=1e-3), colliders=[], cell_width=1.0,
              grid_capacity=1024, model=0)
    shards, part = lockstep_slabs(pipeline(dim), sc, 2)
    assert min(s.num_particles() for s in shards) > 0
    state, held, aff, dist, normal = export_state_and_cdf(shards, ps.n, dim)      # (asserts: every id exactly once)
    for f in ("pos", "vel", "def_grad", "affine", "mass"):
        assert np.array_equal(_bits(state[f]), _bits(getattr(given, f))), f
    from wgsparkl_amd.sharded import associated_block_x
    assert np.array_equal(held, part.owner_of_blocks(associated_block_x(given.pos, 1.0, dim)))
    assert np.array_equal(aff, given.cdf_affinity)
    assert np.array_equal(_bits(np.asarray(dist, np.float32)), _bits(given.cdf_dist))
    assert np.array_equal(_bits(np.asarray(normal, np.float32)), _bits(given.cdf_normal))
    for s in shards:
        s.close()
