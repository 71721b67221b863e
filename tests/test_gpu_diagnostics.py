"""-m gpu: the device-side diagnostics (wgs_read_diagnostics / wgs_enqueue_diagnostics) against tests/diag_truth.py: exact sums on
a dyadic lattice (G1), bounded sums and bounds after 20 substeps (G2), mass / momentum / angular momentum through P2G and the grid
update (G3), bit-identical results across storage orders, launch shapes, restarts and the two entry points (G4), the digest (G5),
non-finite particles (G6), slabs of a decomposition (G7), and that asking changes nothing (G8)."""
import ctypes as C
import math

import numpy as np
import pytest

import diag_truth as dt
from gpu_common import _exploding_cube, cloud_scene
from helpers import BASE_FIELDS, assert_same_bits, assert_same_grid, debug, new_data, pipeline, report_margin, run_gpu, run_oracle
from wgsparkl_amd import _ffi, scenes
from wgsparkl_amd.models import MODEL_COROTATED, MODEL_NEO_HOOKEAN, DruckerPrager
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import SimulationParams

pytestmark = pytest.mark.gpu

ALL = _ffi.DIAG_ALL
U = 2.0 ** -53
# fp64 roundings of one term as the header evaluates it (products of two fp32 values are exact), from the operation count:
#   mass, momentum, mass moment  m, m v, m x: none — 1 is allowed
#   angular      x_a v_b - x_b v_a (1), times m (1), A_ab - A_ba (exact or 1), times D (1), the sum (1): 5
#   kinetic      2 additions of exact squares, times m, times 1/2 (exact): 3
#   affine       8 additions of exact squares, times D, times 1/2 (exact), divided by m: 10
#   gravity      2 additions of exact products, times m: 3
#   elastic      E = G + G^T + G^T G (4 per entry), five Jacobi sweeps of three rotations (about 10 operations on an entry each), square
#                roots and the final sums: the longest chain through an eigenvalue stays below 256 roundings
# the truth is evaluated in fp64 by other code with as many roundings, so twice the count is allowed; all relative to the sum of the
# absolute values of the pieces a term is added up from (diag_truth.terms: `mag`).
ROUNDINGS = dict(mass=1, momentum=1, mass_moment=1, angular=5, kinetic=3, kinetic_affine=10, gravity_potential=3, elastic=256,
                 grid_mass=1, grid_momentum=1, grid_angular=3)
PARTICLE_SUMS = ("mass", "momentum", "angular", "mass_moment", "kinetic", "kinetic_affine", "gravity_potential", "elastic")


def _new(sc):
    return new_data(sc)[1]


def _check_sums(tag, d, got, sc, quality=True):
    """Every particle sum of `d` against the fp64 truth of the read-back `got`: |value - truth| <= N 2^(exponent-1) + evaluation error;
    and the exponent is good enough that N 2^(exponent-1) <= 2^-24 sum |term|."""
    t, mag = dt.terms(got, sc["cell_width"], sc["params"].gravity, sc.get("model", 0), energy=True)
    n = d.num_particles
    for name in PARTICLE_SUMS:
        s = d.sums[name]
        for k in range(t[name].shape[1]):
            truth = math.fsum(t[name][:, k])
            rounding = n * 2.0 ** (s.exponent - 1)
            evaluation = 2 * ROUNDINGS[name] * U * math.fsum(mag[name][:, k])
            err = abs(float(s.value[k]) - truth)
            report_margin(f"{tag} {name}[{k}] |value - truth|", err, rounding + evaluation, exponent=s.exponent)
            assert err <= rounding + evaluation, (tag, name, k, err, rounding, evaluation)
            assert s.value[k] == math.ldexp(int(s.fixed[k]), s.exponent)
        total = math.fsum(np.abs(t[name]).max(1))
        if quality:
            report_margin(f"{tag} {name} rounding bound / sum|term|", n * 2.0 ** (s.exponent - 1) / total, 2.0 ** -24)
            assert n * 2.0 ** (s.exponent - 1) <= 2.0 ** -24 * total, (tag, name)
        assert abs(int(np.abs(s.fixed).max())) < 2 ** 62


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(float(a) - float(b)) / float(np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)))


def _check_bounds(tag, d, got, sc):
    """Pure max / min of stored values: exact. Computed values (fp64, rounded to fp32 once on the device; fp64 numpy rounded here):
    1 ulp for the double rounding; det F, a sum of products that cancel, 2 ulp of the LARGEST product instead."""
    b = dt.bounds(got, sc["cell_width"], sc["params"].dt)
    assert np.array_equal(d.aabb_min, b["aabb_min"]) and np.array_equal(d.aabb_max, b["aabb_max"])
    assert np.float32(d.cfl) == b["cfl"], (d.cfl, b["cfl"])
    for name in ("max_speed", "max_affine_norm", "max_wave_speed"):
        u = _ulps(getattr(d, name), b[name])
        report_margin(f"{tag} {name} ulps", u, 1.0)
        assert u <= 1.0, (name, getattr(d, name), b[name])
    scale = float(np.spacing(np.float32(np.max(np.abs(got.def_grad)) ** got.dim)))
    for name, ref in (("min_det_f", b["det"].min()), ("max_det_f", b["det"].max())):
        err = abs(float(getattr(d, name)) - ref)
        report_margin(f"{tag} {name}", err, 2 * scale)
        assert err <= 2 * scale, (name, getattr(d, name), ref)


def _dyadic(ps, seed):
    rng = np.random.default_rng(seed)
    q = lambda shape, lo: (rng.integers(lo, 1025, shape) / 256.0).astype(np.float32)
    ps.pos[:], ps.vel[:], ps.mass[:] = q(ps.pos.shape, 400), q(ps.vel.shape, -1024), q(ps.mass.shape, 1)


@pytest.mark.parametrize("dim", [2, 3])
def test_exact_sums_on_a_dyadic_lattice(dim):
    """G1: masses, positions and velocities k / 256 with |k| <= 1024, h = 1, no substep: `fixed` and `exponent` of mass, momentum and
    mass moment equal the Python-integer truth exactly."""
    sc = cloud_scene(n=5000, dim=dim)
    _dyadic(sc["particles"], 11 + dim)
    d = _new(sc).diagnostics(_ffi.DIAG_PARTICLES)
    truth = dt.exact_sums(sc["particles"], sc["cell_width"], sc["params"].gravity, energy=False)
    assert d.num_particles == 5000 and d.num_nonfinite == 0
    for name in ("mass", "momentum", "mass_moment"):
        fixed, e = truth[name]
        assert d.sums[name].exponent == e, name
        assert [int(x) for x in d.sums[name].fixed] == fixed, name


def _scene(kind):
    if kind == "corotated3":
        return cloud_scene(n=6000, dim=3, model=MODEL_COROTATED)
    if kind == "neohookean3":
        return cloud_scene(n=6000, dim=3, model=MODEL_NEO_HOOKEAN, seed=9)
    if kind == "neohookean2":
        return cloud_scene(n=6000, dim=2, model=MODEL_NEO_HOOKEAN, seed=10)
    if kind == "corotated2":
        return cloud_scene(n=6000, dim=2, model=MODEL_COROTATED, seed=12)
    dim = 3 if kind == "sand3" else 2
    ps = scenes.random_cloud(6000, dim=dim, seed=21, young=1e6, plasticity=DruckerPrager.new(1e6, 0.25), phase=None, perturb_F=0.02,
                             perturb_C=0.2)
    return dict(particles=ps, params=SimulationParams((0.0, -9.81, 0.0)[:dim], 8e-4), colliders=[], cell_width=1.0, grid_capacity=4096,
                model=MODEL_COROTATED)


@pytest.mark.parametrize("kind", ["corotated3", "neohookean3", "neohookean2", "corotated2", "sand3"])
def test_sums_and_bounds_after_twenty_substeps(kind):
    """G2: every sum within N 2^(exponent-1) + the fp64 evaluation error of its terms (ROUNDINGS above) of the fp64 truth computed from
    wgs_read_particles of the same state; the exponent leaves at most 2^-24 of sum |term|; bounds exact or within the stated ulps."""
    sc = _scene(kind)
    data = run_gpu(sc, 20)
    d = data.diagnostics(ALL)
    got = data.read_particles()
    assert d.num_particles == got.n and d.num_nonfinite == 0 and d.model == sc["model"] and d.what == ALL
    if kind == "sand3":
        assert (got.dp_state != np.array([1.0, 1.0, 0.0], np.float32)).any(), "the sand should have yielded"
    _check_sums(kind, d, got, sc)
    _check_bounds(kind, d, got, sc)
    # the grid sums against wgs_read_grid of the same state
    cells, vm = data.read_grid()[:2]
    gt, gmag = dt.grid_terms(cells, vm, sc["cell_width"], got.dim)
    for name, col in gt.items():
        s = d.sums[name]
        for k in range(col.shape[1]):
            bound = len(cells) * 2.0 ** (s.exponent - 1) + 2 * ROUNDINGS[name] * U * math.fsum(gmag[name][:, k])
            err = abs(float(s.value[k]) - math.fsum(col[:, k]))
            report_margin(f"{kind} {name}[{k}] |value - truth|", err, bound)
            assert err <= bound, (name, k, err, bound)
    assert d.suggest_dt(sc["params"].dt, 0.5) == pytest.approx(0.5 * sc["params"].dt / d.cfl)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("gravity", [True, False])
def test_grid_sums_continue_the_particle_sums(dim, gravity):
    """G3: no collider, one substep. GRID_MASS = MASS, GRID_MOMENTUM = MOMENTUM(before) + MASS g dt, and with g = 0 GRID_ANGULAR =
    ANGULAR(before) — which pins sign and scale of the affine term. Allowed: the two sums' own bounds plus the fp32 rounding of P2G
    and the grid update, MEASURED on the fp32 oracle (the same three differences from its particles and grid): the larger of 4 x the
    oracle's own discrepancy (helpers.py k32) and 1e-5 of sum |term| (helpers.py grid tolerance)."""
    sc = cloud_scene(n=6000, dim=dim, seed=31 + dim)
    g = np.array((0.0, -9.81, 0.0)[:dim] if gravity else (0.0,) * dim)
    sc["params"] = SimulationParams(tuple(g), 1.0e-3)
    ps, h, dtm = sc["particles"], sc["cell_width"], 1.0e-3
    data = _new(sc)
    before = data.diagnostics(_ffi.DIAG_PARTICLES)
    pipeline(dim).step(data, 1)
    data.sync()
    after = data.diagnostics(_ffi.DIAG_GRID)
    n, nodes = before.num_particles, len(data.read_grid()[0])
    # the fp32 oracle's own discrepancies, in fp64 from its inputs and its grid
    st = run_oracle(sc, 1, np.float32)
    ocells, ovm = st.grid_records()[:2]
    og, _ = dt.grid_terms(ocells, ovm, h, dim)
    pt, _ = dt.terms(ps, h, g, energy=False)
    mass0 = math.fsum(pt["mass"][:, 0])
    expect = dict(grid_mass=[mass0], grid_momentum=[math.fsum(pt["momentum"][:, k]) + mass0 * g[k] * dtm for k in range(dim)],
                  grid_angular=[math.fsum(pt["angular"][:, k]) for k in range(pt["angular"].shape[1])])
    checks = [("grid_mass", "mass"), ("grid_momentum", "momentum")] + ([] if gravity else [("grid_angular", "angular")])
    for gname, pname in checks:
        gs, psum = after.sums[gname], before.sums[pname]
        for k in range(len(expect[gname])):
            oracle_gap = abs(math.fsum(og[gname][:, k]) - expect[gname][k])
            scale = math.fsum(np.abs(og[gname][:, k]))
            p2g = max(4.0 * oracle_gap, 1.0e-5 * scale)
            want = float(psum.value[k]) + (float(before.sums["mass"].value[0]) * g[k] * dtm if gname == "grid_momentum" else 0.0)
            bound = n * 2.0 ** (psum.exponent - 1) + nodes * 2.0 ** (gs.exponent - 1) + p2g
            err = abs(float(gs.value[k]) - want)
            report_margin(f"{gname}[{k}] dim {dim} gravity {gravity}: vs 4 x fp32 oracle gap", err, 4.0 * oracle_gap + bound - p2g)
            report_margin(f"{gname}[{k}] dim {dim} gravity {gravity}: vs 1e-5 sum|term|", err, 1.0e-5 * scale + bound - p2g)
            assert err <= bound, (gname, k, err, bound, oracle_gap, scale)


def _sand(dim=3):
    sc = _scene("sand3" if dim == 3 else "sand2")
    sc["particles"].vel[:] *= 3.0
    return sc


def test_reproducible_across_runs_shapes_restarts_and_entry_points(monkeypatch):
    """G4: the complete struct is bit-identical (a) between two runs of a stirred scene (block ids are dealt by atomics), (b) between
    the shipped launch shapes and WGS_DEBUG NO_UNIFORM / NO_DIRECT_RUNS, (c) between a continuous run and read-back -> create ->
    set_plastic_state -> continue, (d) between wgs_read_diagnostics and wgs_enqueue_diagnostics + a copy."""
    import torch

    def run(make, steps=30):
        data = run_gpu(make(), steps)
        return data, data.diagnostics(ALL)
    # (a), (b)
    for make in (_exploding_cube, _sand):
        _, a = run(make)
        _, a2 = run(make)
        assert a.raw == a2.raw
        assert a.num_particles > 0 and a.digest != (0, 0)
        for switch in ("NO_UNIFORM", "NO_DIRECT_RUNS"):
            with debug(monkeypatch, switch):
                _, b = run(make)
            assert a.raw == b.raw, switch
    # (c)
    whole, a = run(_sand, 20)
    first = run_gpu(_sand(), 10)
    mid = first.read_particles()
    sc = _sand()
    sc["particles"] = mid
    again = _new(sc)
    again.set_plastic_state(mid.dp_state)
    pipeline(3).step(again, 10)
    again.sync()
    assert again.diagnostics(ALL).raw == a.raw
    # (d)
    buf = torch.zeros(C.sizeof(_ffi.Diagnostics), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    whole.enqueue_diagnostics(buf.data_ptr(), ALL)
    whole.sync()
    assert bytes(buf.cpu().numpy().tobytes()) == a.raw


@pytest.mark.parametrize("kind", ["corotated3", "neohookean2", "sand3", "sand2"])
def test_digest_is_the_header_hash_of_the_read_back(kind):
    """G5: digest == diag_truth.digest(read_particles()) in 2D and 3D, elastic and plastic; one velocity bit of one particle changes it."""
    sc = _scene(kind)
    data = run_gpu(sc, 12)
    d = data.diagnostics(_ffi.DIAG_DIGEST)
    got = data.read_particles()
    assert d.digest == dt.digest(got) and d.num_particles == got.n
    assert d.what == _ffi.DIAG_DIGEST and all(float(s.value[0]) == 0.0 for s in d.sums.values())
    flipped = _scene(kind)
    v = flipped["particles"].vel.view(np.uint32)
    v[137, 0] ^= np.uint32(1)
    a, b = _new(sc).diagnostics(_ffi.DIAG_DIGEST), _new(flipped).diagnostics(_ffi.DIAG_DIGEST)
    assert a.digest == dt.digest(_new(sc).read_particles())
    assert a.digest[0] != b.digest[0] and a.digest[1] != b.digest[1]


def _lone_slab(ps, ids, sc):
    from wgsparkl_amd.sharded import INT_MAX, INT_MIN, NativeShard
    return NativeShard(pipeline(ps.dim), sc["params"], ps, ids, [], sc["cell_width"], sc["grid_capacity"], INT_MIN, INT_MAX, False, False,
                       particle_capacity=ps.n, model=sc["model"], force_plastic=True)


def test_digest_ignores_the_upload_order():
    """G5: the same particles under the same ids, uploaded in shuffled order (a slab carries the ids it is given), give the same
    digest — and the same sums, bit for bit."""
    sc = cloud_scene(n=4000, dim=3)
    ps = sc["particles"]
    ids = np.arange(ps.n, dtype=np.uint32)
    perm = np.random.default_rng(2).permutation(ps.n)
    shuffled = type(ps)(**{k: (v[perm] if isinstance(v, np.ndarray) else v) for k, v in ps.__dict__.items()})
    a = _lone_slab(ps, ids, sc).diagnostics(ALL)
    b = _lone_slab(shuffled, ids[perm], sc).diagnostics(ALL)
    assert a.raw == b.raw
    assert a.digest == dt.digest(ps)


def test_non_finite_particles_are_counted_and_left_out():
    """G6: a particle with a NaN velocity component is counted and left out of every sum and bound; the other sums are those of the
    cloud without it. No substep is run: NaN arithmetic inside the diagnostics only."""
    sc = cloud_scene(n=3000, dim=3)
    ps = sc["particles"]
    clean = type(ps)(**{k: (np.delete(v, 77, 0) if isinstance(v, np.ndarray) else v) for k, v in ps.__dict__.items()})
    ps.vel[77, 1] = np.nan
    d = _new(sc).diagnostics(_ffi.DIAG_PARTICLES | _ffi.DIAG_ENERGY)
    sc2 = dict(sc, particles=clean)
    ref = _new(sc2).diagnostics(_ffi.DIAG_PARTICLES | _ffi.DIAG_ENERGY)
    assert (d.num_particles, d.num_nonfinite) == (3000, 1) and (ref.num_particles, ref.num_nonfinite) == (2999, 0)
    for name in PARTICLE_SUMS:      # (3000 and 2999 have the same number of bits: the same exponents)
        assert d.sums[name].exponent == ref.sums[name].exponent and np.array_equal(d.sums[name].fixed, ref.sums[name].fixed), name
        assert np.all(np.isfinite(d.sums[name].value))
    for name in ("max_speed", "max_affine_norm", "min_det_f", "max_det_f", "max_wave_speed", "cfl"):
        assert getattr(d, name) == getattr(ref, name), name
    assert np.array_equal(d.aabb_min, ref.aabb_min) and np.array_equal(d.aabb_max, ref.aabb_max)


@pytest.mark.parametrize("world", [2, 3])
def test_slabs_add_up_to_the_single_domain(world):
    """G7: 2 and 3 lockstep slabs after a few substeps: the counts add up to N, the digests add up (mod 2^64) to the numpy digest of
    the concatenated export_records() of the slabs, mass and momentum add up to the single-domain run's within the sums' bounds + 1e-5."""
    from wgsparkl_amd.sharded import native_lockstep, record_quad, unpack_records
    sc = cloud_scene(n=12000, dim=3, extent=30.0)
    pipe = pipeline(3)
    shards, _ = lockstep_slabs(pipe, sc, world, force_plastic=True)
    native_lockstep(pipe, shards, 6)
    for s in shards:
        s.sync()
    ds = [s.diagnostics(ALL) for s in shards]
    assert sum(d.num_particles for d in ds) == sc["particles"].n
    hashes = []
    for s in shards:
        rec = s.export_records()
        r = unpack_records(rec, 3, s.uniform_material)
        dp1, dp2 = record_quad(rec, 3, "DP1"), record_quad(rec, 3, "DP2")
        state = np.concatenate([dp1[:, 2:4], dp2[:, 0:1]], 1)            # layout.h: DP1 = (.., .., st0, st1), DP2 = (st2, phase, max_stretch, -)
        phase = dp2[:, 1:3]
        words = np.concatenate([np.ascontiguousarray(a, np.float32).view(np.uint32) for a in
                                (r["pos"], r["vel"], r["def_grad"], r["affine"], state, phase)], 1)
        hashes.append(dt.particle_hashes(r["ids"], words))
    want = dt.digest_of_hashes(np.concatenate(hashes))
    mod = 1 << 64
    assert (sum(d.digest[0] for d in ds) % mod, sum(d.digest[1] for d in ds) % mod) == want
    for d, h in zip(ds, hashes):
        assert d.digest == dt.digest_of_hashes(h)
    single_data = run_gpu(sc, 6)
    single = single_data.diagnostics(ALL)
    got = single_data.read_particles()
    assert single.digest == dt.digest(got)
    t, _ = dt.terms(got, sc["cell_width"], sc["params"].gravity, energy=False)
    for name in ("mass", "momentum"):
        for k in range(t[name].shape[1]):
            bound = sum(d.num_particles * 2.0 ** (d.sums[name].exponent - 1) for d in ds + [single]) + 1.0e-5 * math.fsum(np.abs(t[name][:, k]))
            err = abs(sum(float(d.sums[name].value[k]) for d in ds) - float(single.sums[name].value[k]))
            report_margin(f"{world} slabs {name}[{k}] vs single domain", err, bound)
            assert err <= bound, (name, k, err, bound)


def test_asking_changes_nothing():
    """G8: diagnostics between the steps leave wgs_read_particles bit-identical to a run that never asked (they read the right side of
    the ping-pong and write no state)."""
    def run(ask):
        sc = _sand()
        data = _new(sc)
        pipe = pipeline(3)
        seen = []
        for k in (5, 6, 7):
            pipe.step(data, k)
            if ask:
                seen.append(data.diagnostics(ALL))
        data.sync()
        return data.read_particles(), data.read_grid(), seen
    a, ga, seen = run(True)
    b, gb, _ = run(False)
    assert_same_bits(a, b, BASE_FIELDS + ("dp_state", "phase", "mass"))
    assert_same_grid(ga, gb)
    assert len({d.raw for d in seen}) == 3 and seen[-1].digest == dt.digest(a)
