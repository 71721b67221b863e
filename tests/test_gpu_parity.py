"""-m gpu: the HIP path through the C ABI against the oracle (fp64 truth, fp32 twin) — single substeps, the BASELINE.json configurations at test
size, the reference's own scenes, random scenes and API sequences, the committed golden vectors, the C ABI's error behaviour. Integer results
(cells, blocks, membership, node bits) exact; floating point within the tolerances of tests/gpu_common.py."""
import numpy as np
import pytest

from wgsparkl_amd import KernelInvocationQueue, _ffi, scenes
from wgsparkl_amd.models import (MODEL_COROTATED, MODEL_NEO_HOOKEAN, DruckerPrager, ElasticCoefficients, ParticlePhase)
from wgsparkl_amd.solver import Collider, ParticleSet, SimulationParams

from helpers import (AFFINITY_FIELDS, BASE_FIELDS, assert_close_to_truth, assert_same_bits, assert_same_bodies, compare_cpic, compare_grids, debug,
                     grid_of, new_data, oracle, pipeline, rel_rms, report_margin, run_gpu, run_oracle, step_chunks)
from gpu_common import (CPIC_GRID_V_TOL, CPIC_PART_TOL, FUZZ_BODY_ATOL, FUZZ_NODE_MISMATCH, FUZZ_PART_MISMATCH, FUZZ_VEL_TOL, GRID_V_TOL, PART_TOL,
                        _exploding_cube, _random_scene, check_blocks, check_fields, check_grid, cloud_scene)
import os as _os

from golden_cases import CASES as _CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model", [MODEL_COROTATED, MODEL_NEO_HOOKEAN])
def test_one_substep_cloud_3d(hip_libs, oracle_libs, model):
    sc = cloud_scene(model=model)
    data = run_gpu(sc, 1)
    st32 = run_oracle(sc, 1, np.float32)
    st64 = run_oracle(sc, 1, np.float64)
    check_blocks(data, st32)
    check_grid(data, st32, st64)
    check_fields(data, st32, st64)


def test_reference_smoke_scene(hip_libs, oracle_libs):
    """The reference's own pipeline_queue_step scene (src/pipeline.rs:302-333): 3 substeps,
    phase None + plasticity None => Drucker-Prager with lambda = mu = -1 (quirk B1)."""
    sc = scenes.reference_smoke_scene()
    data = run_gpu(sc, 3)
    st32 = run_oracle(sc, 3, np.float32)
    st64 = run_oracle(sc, 3, np.float64)
    check_blocks(data, st32)
    check_grid(data, st32, st64)
    check_fields(data, st32, st64)


@pytest.mark.parametrize("k", [10])
def test_multi_substep_cube(hip_libs, oracle_libs, k):
    sc = scenes.neo_hookean_cube(n_side=24)
    data = run_gpu(sc, k)
    st64 = run_oracle(sc, k, np.float64)
    st32 = run_oracle(sc, k, np.float32)
    check_blocks(data, st32)
    check_grid(data, st32, st64)
    check_fields(data, st32, st64)


@pytest.mark.parametrize("with_floor", [False, True])
def test_c5_fluid_block_small(hip_libs, oracle_libs, with_floor):
    """configs[4] at a size the oracle finishes in seconds: the pressure-only neo-Hookean "fluid" (mu = 0,
    neo_hookean_elasticity.wgsl:14-25), compressed and sheared so that the pressure term acts, 10 substeps; without
    the floor to the north_star tolerance (grid velocity 1e-5 vs the fp64 oracle, cells exact), with the block lying on
    the floor through the CPIC passes."""
    sc = scenes.fluid_block(40, 24, 24, with_floor=with_floor)
    ps = sc["particles"]
    rng = np.random.default_rng(55)
    ps.vel[:] = rng.normal(0, 0.4, ps.vel.shape).astype(np.float32)
    ps.def_grad[:] += rng.normal(0, 0.03, ps.def_grad.shape).astype(np.float32)
    ps.def_grad[:, [0, 4, 8]] *= np.float32(0.97)                       # ln J < 0: the fluid pushes back
    if with_floor:
        ps.pos[:, 1] -= 5.7                                               # lowest particles inside the floor's reach
    k = 10
    data = run_gpu(sc, k)
    st32 = run_oracle(sc, k, np.float32)
    st64 = run_oracle(sc, k, np.float64)
    check_blocks(data, st32)
    if not with_floor:
        check_grid(data, st32, st64)
        check_fields(data, st32, st64)
    else:
        got, same = compare_cpic(data, st32, st64, 3, CPIC_GRID_V_TOL, CPIC_PART_TOL, min_same=0.998)
        assert (got.cdf_affinity & 1).sum() > 500                        # the floor is felt


def test_drucker_prager_sand(hip_libs, oracle_libs):
    sc = scenes.sand_column(nx=16, ny=24, nz=16)
    ps = sc["particles"]
    rng = np.random.default_rng(3)
    ps.vel[:] = rng.normal(0, 0.5, ps.vel.shape).astype(np.float32)
    ps.def_grad[:] += rng.normal(0, 0.02, ps.def_grad.shape).astype(np.float32)
    sc["params"] = SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0e-4)
    data = run_gpu(sc, 2)
    st64 = run_oracle(sc, 2, np.float64)
    st32 = run_oracle(sc, 2, np.float32)
    got = check_fields(data, st32, st64, tol=1e-4)
    assert_close_to_truth("dp_state", got.dp_state, st32.arr["dp_state"], st64.arr["dp_state"], 1e-4)


def test_2d_block(hip_libs, oracle_libs):
    sc = scenes.elastic_block_2d(nx=40, ny=40, with_floor=False)
    data = run_gpu(sc, 5)
    st32 = run_oracle(sc, 5, np.float32)
    st64 = run_oracle(sc, 5, np.float64)
    check_blocks(data, st32)
    check_grid(data, st32, st64, dim=2)
    check_fields(data, st32, st64)


@pytest.mark.parametrize("landed", [False, True])
def test_c1_configs0_as_written(hip_libs, oracle_libs, landed):
    """BASELINE.json configs[0] at its full size: the 2D elastic block of 100 x 100 = 10 000 particles (4 per cell,
    crates/wgsparkl2d/examples/elasticity2.rs:33-55 conventions) over the floor cuboid, 100 substeps, against the fp64
    oracle with the CPIC tolerances (the floor makes it a collider simulation). As written the block is still falling
    after 100 substeps; `landed` lowers it onto the floor so that the same 100 substeps go through contact."""
    sc = scenes.elastic_block_2d(nx=100, ny=100, with_floor=True)
    assert sc["particles"].n == 10_000
    if landed:
        sc["particles"].pos[:, 1] -= 5.0
        sc["particles"].vel[:, 1] = -2.0
    k = 100
    data = run_gpu(sc, k)
    st32 = run_oracle(sc, k, np.float32)
    st64 = run_oracle(sc, k, np.float64)
    check_blocks(data, st32)
    got, same = compare_cpic(data, st32, st64, 2, CPIC_GRID_V_TOL, CPIC_PART_TOL, min_same=0.998)
    if landed:
        assert (got.cdf_affinity & 1).sum() >= 300, "the floor must be felt"
        assert np.abs(got.def_grad - np.eye(2, dtype=np.float32).reshape(-1)).max() > 1e-3, "the block must deform"


def test_reference_sand3_scene_as_shipped(hip_libs, oracle_libs):
    """The reference's own shipping scene (crates/wgsparkl3d/examples/sand3.rs:28-113) at its full size — 202 500
    Drucker-Prager particles, floor, four walls, the tilted kinematic cuboid spinning under the column — 6 substeps against
    the fp64 oracle: blocks and node bits exact, fields to the collider-scene tolerances, the body pose too."""
    sc = scenes.reference_sand3()
    assert sc["particles"].n == 202_500
    k = 6
    data = run_gpu(sc, k)
    st32 = run_oracle(sc, k, np.float32)
    st64 = run_oracle(sc, k, np.float64)
    check_blocks(data, st32)
    got, same = compare_cpic(data, st32, st64, 3, CPIC_GRID_V_TOL, 1e-4, min_same=0.998, fields=("pos", "vel", "def_grad"))
    assert (got.cdf_affinity != 0).sum() > 100, "the spinning cuboid must be felt"
    pose = data.read_body_poses()[5]
    want = st64.collider_states()[5]
    assert np.allclose(pose["rotation"], want["rotation"], atol=1e-6) and np.allclose(pose["translation"], want["translation"], atol=1e-6)


def test_empty_and_single(hip_libs, oracle_libs):
    sc = cloud_scene(n=1)
    data = run_gpu(sc, 2)
    st64 = run_oracle(sc, 2, np.float64)
    check_fields(data, run_oracle(sc, 2, np.float32), st64)
    sc0 = cloud_scene(n=1)
    sc0["particles"] = ParticleSet.uniform(np.zeros((0, 3), np.float32), 0.25, 1.0, ElasticCoefficients(1.0, 1.0))
    d0 = run_gpu(sc0, 2)
    assert d0.read_positions().shape == (0, 3)


@pytest.mark.parametrize("dim", [3, 2])
def test_reference_prefix_sum_vectors_through_the_hip_scan(hip_libs, oracle_libs, dim):
    """The ONLY numeric answers the reference's own tests hold for this path — gpu_prefix_sum,
    src/grid/prefix_sum.rs:183-229: all-ones, iota and random % 10_000 at LEN = 15071 — put through the device scan
    that replaces WgPrefixSum (kernels_sort.h scan_chunk, via the wgs_debug_scan hook): out[i] = i, out[i] = i(i-1)/2,
    and equality with eval_cpu (restated in the oracle). Plus the edge lengths around the chunk and wave sizes."""
    import ctypes as C
    pipe = pipeline(dim)
    orc = oracle_libs.Oracle(3, np.float32)

    def hip_scan(v):
        v = np.ascontiguousarray(v, np.uint32)
        out = np.zeros(len(v), np.uint32)
        tot = C.c_uint32(0)
        u32p = C.POINTER(C.c_uint32)
        _ffi.check(pipe.lib, pipe.lib.wgs_debug_scan(pipe._h, v.ctypes.data_as(u32p), len(v), out.ctypes.data_as(u32p), C.byref(tot)))
        return out, tot.value

    n = 15071
    ones, iota = np.ones(n, np.uint32), np.arange(n, dtype=np.uint32)
    rnd = (np.random.default_rng(0).integers(0, 2**32, n, dtype=np.uint64) % 10_000).astype(np.uint32)
    out, tot = hip_scan(ones)
    assert np.array_equal(out, np.arange(n, dtype=np.uint32)) and tot == n
    out, tot = hip_scan(iota)
    i = np.arange(n, dtype=np.uint64)
    assert np.array_equal(out, ((i * (i - 1)) // 2).astype(np.uint32))
    for v in (ones, iota, rnd):
        out, tot = hip_scan(v)
        assert np.array_equal(out, orc.prefix_sum_eval_cpu(v)) and tot == int(v.astype(np.uint64).sum() & 0xffffffff)
    for m in (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 65536, 65537, 300001):
        v = ((np.arange(m, dtype=np.uint64) * 7 + 3) % 11).astype(np.uint32)
        out, tot = hip_scan(v)
        assert np.array_equal(out, orc.prefix_sum_eval_cpu(v)) if m else len(out) == 0
        assert tot == int(v.sum())


def test_dense_blocks_take_the_global_memory_paths_of_the_sort(hip_libs, oracle_libs):
    """A wave of the sort's second launch stages a block's previous run and its new order in LDS, 768 entries each
    (kernels_sort.h RUNCAP); denser blocks go through the same code on global memory. 27 particles per cell = 1728 per
    block, moving fast enough to change cells and blocks every few substeps: against the oracle (cells and per-block
    membership exact, fields to tolerance), deterministic, and bit-identical to full binning on every substep."""
    h = 1.0
    n = 36
    ax = (np.arange(n, dtype=np.float64) + 0.5) * (h / 3.0) + 6.0
    pos = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(77)
    pos = (pos + rng.uniform(-0.04, 0.04, pos.shape)).astype(np.float32)
    ps = ParticleSet.uniform(pos, h / 6.0, 50.0, ElasticCoefficients.from_young_modulus(1.0e5, 0.3), phase=ParticlePhase(1.0, -1.0))
    ps.vel[:] = rng.normal(0.0, 40.0, ps.vel.shape).astype(np.float32)            # ~0.04 cells per substep
    sc = dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0e-3), colliders=[], cell_width=h,
              grid_capacity=1024, model=MODEL_NEO_HOOKEAN)
    k = 12
    data = run_gpu(sc, k)
    st32, st64 = run_oracle(sc, k, np.float32), run_oracle(sc, k, np.float64)
    vid, first, num, ids = data.read_blocks()
    assert num.max() > 768, "the scene must exceed the LDS stage"
    check_blocks(data, st32)
    check_grid(data, st32, st64)
    check_fields(data, st32, st64)
    a = data.read_particles()
    b = run_gpu(sc, k).read_particles()
    assert_same_bits(a, b, BASE_FIELDS)


def test_visit_list_many_listed_blocks_per_chunk(hip_libs, oracle_libs, monkeypatch):
    """The CPIC body of the fused G2P advances a visit list: one entry per (block near a collider, chunk of 64 sorted
    particles holding some of its particles), dealt to eight lists (kernels_sort.h / device_math.h append_visits). A thin,
    sparse sheet of particles over a floor — two or three particles per block, a few hundred listed blocks, so every chunk
    holds dozens of listed blocks and is visited once for each — next to a compact clump (blocks spanning several chunks):
    against the oracle, and bit-identical with two and with one chunk per wave of the main body (other list groupings)."""
    h = 1.0
    rng = np.random.default_rng(91)
    sheet = np.stack([rng.uniform(4.0, 90.0, 700), rng.uniform(2.3, 3.4, 700), rng.uniform(4.0, 90.0, 700)], -1)
    ax = (np.arange(16, dtype=np.float64) + 0.5) * (h / 2.0) + 40.0
    clump = np.stack(np.meshgrid(ax, (np.arange(10) + 0.5) * (h / 2.0) + 2.3, ax, indexing="ij"), -1).reshape(-1, 3)
    pos = np.concatenate([sheet, clump + rng.uniform(-0.05, 0.05, clump.shape)]).astype(np.float32)
    ps = ParticleSet.uniform(pos, h / 4.0, 1000.0, ElasticCoefficients.from_young_modulus(2.0e5, 0.3), phase=ParticlePhase(1.0, -1.0))
    ps.vel[:] = rng.normal(0.0, 1.0, ps.vel.shape).astype(np.float32)
    ps.vel[:, 1] -= 3.0
    sc = dict(particles=ps, params=SimulationParams(gravity=(0.0, -9.81, 0.0), dt=1.0e-3),
              colliders=[Collider.cuboid((1000.0, 2.0, 1000.0), (0.0, 0.0, 0.0))], cell_width=h, grid_capacity=4096, model=MODEL_NEO_HOOKEAN)
    k = 12
    data = run_gpu(sc, k)
    st = data.stats()
    assert st["num_near_collider_blocks"] > 300 and st["num_near_collider_blocks"] * 64 > ps.n   # far more listed blocks than chunks
    st32, st64 = run_oracle(sc, k, np.float32), run_oracle(sc, k, np.float64)
    check_blocks(data, st32)
    got, same = compare_cpic(data, st32, st64, 3, CPIC_GRID_V_TOL, CPIC_PART_TOL, min_same=0.995)
    assert (got.cdf_affinity & 1).sum() > 500
    with debug(monkeypatch, "G2P_TWO_PASSES"):
        b = run_gpu(sc, k).read_particles()
        assert_same_bits(got, b, AFFINITY_FIELDS)


def test_device_ptrs_view_matches_the_read_back(hip_libs):
    """wgs_get_device_ptrs (the optional interop view of SURVEY 8b): the position quads and particle ids it points at, copied
    straight from device memory, are the positions wgs_read_positions returns — in sorted order, labelled by the ids."""
    import ctypes as C
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=True)
    pipe, data = new_data(sc)
    step_chunks(data, (7,))
    view = _ffi.DevicePtrs()
    _ffi.check(pipe.lib, pipe.lib.wgs_get_device_ptrs(data._h, C.byref(view)))
    n = sc["particles"].n
    assert view.count == n and view.capacity >= n and view.dim == 3 and view.position_quads and view.particle_ids
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    quads = np.empty((n, 4), np.float32)
    ids = np.empty(n, np.uint32)
    assert hip.hipMemcpy(quads.ctypes.data, view.position_quads, quads.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    assert hip.hipMemcpy(ids.ctypes.data, view.particle_ids, ids.nbytes, 2) == 0
    assert np.array_equal(np.sort(ids), np.arange(n, dtype=np.uint32))
    pos = data.read_particles().pos
    assert np.array_equal(quads[:, :3], pos[ids])


def test_grid_overflow_is_reported(hip_libs):
    sc = cloud_scene(n=5000)
    sc["grid_capacity"] = 8
    with pytest.raises(_ffi.WgsError):
        run_gpu(sc, 1)


def test_grid_grows_before_it_overflows(hip_libs):
    """SURVEY 8f4, second half (the reference's resize loop is a stub, src/grid/grid.rs:43-45,116-117): a scene whose
    active blocks outgrow the capacity it was created with. With growth (the default) the capacity doubles between
    wgs_step calls and the run is bit-identical to one that had a large capacity from the start; with growth switched
    off the overflow is reported, as before."""
    def run(cap, grow, frames=30, per=10):
        pipe, data = new_data(_exploding_cube(), grid_capacity=cap)
        _ffi.check(pipe.lib, pipe.lib.wgs_set_grid_growth(data._h, 1 if grow else 0))
        for _ in range(frames):
            pipe.step(data, per)           # asynchronous: the growth check looks at what the PREVIOUS call left behind
        data.sync()
        return data

    big = run(4096, True)
    assert big.stats()["grid_growths"] == 0 and big.stats()["num_active_blocks"] > 64
    small = run(64, True)
    st = small.stats()
    assert st["overflow"] == 0 and st["grid_growths"] >= 1 and st["grid_capacity"] > 64
    assert_same_bits(big.read_particles(), small.read_particles(), BASE_FIELDS)
    with pytest.raises(_ffi.WgsError):
        run(64, False)


def test_fast_translation_needs_no_more_capacity_than_its_active_blocks(hip_libs):
    """Physical block ids persist between table rebuilds, so a body that moves fast touches, within the 64-substep
    rebuild period, many more blocks than are ever active at once. The capacity bounds the ACTIVE blocks (like the
    reference's, which rebuilds its table every substep): the table is rebuilt early when three quarters of the ids are
    handed out, instead of reporting an overflow."""
    sc = scenes.neo_hookean_cube(n_side=16)
    sc["particles"].vel[:, 0] = 900.0                               # 0.75 cells per substep
    sc["params"] = SimulationParams(gravity=(0.0, 0.0, 0.0), dt=sc["params"].dt)
    pipe, data = new_data(sc, colliders=[], grid_capacity=128)   # 64 active blocks
    _ffi.check(pipe.lib, pipe.lib.wgs_set_grid_growth(data._h, 0))
    for _ in range(40):
        pipe.step(data, 4)
    data.sync()                                                     # raises on WGS_ERR_GRID_OVERFLOW
    st = data.stats()
    assert st["overflow"] == 0 and st["grid_capacity"] == 128 and st["num_active_blocks"] <= 64
    got = data.read_particles()
    assert np.allclose(got.vel[:, 0], 900.0, rtol=1e-5) and np.abs(got.def_grad - np.eye(3, dtype=np.float32).reshape(-1)).max() < 1e-4


@pytest.mark.parametrize("seed,chunk", [(s, 0) for s in range(24)] + [(s, 3) for s in (1, 4, 7, 10, 13, 16, 19, 22)])
def test_random_scenes_match_oracle(hip_libs, oracle_libs, seed, chunk):
    """Fuzz-style parity: random materials and random collider sets (all shape kinds, kinematic and dynamic),
    12 substeps, against the fp32 oracle (same arithmetic): active cells and node affinity / sign bits exact,
    bodies and particles within fp32 round-off growth. chunk = 3: the same substeps in four calls with a wgs_sync
    after each, so that the launch shapes that follow the near-collider list the host last saw are the ones compared."""
    _fuzz_parity(_random_scene(seed), chunk)


def _breakable_scene(seed):
    """_random_scene(seed) (its random stream untouched) with every particle made plastic and breakable: Drucker-Prager
    sand parameters and phase (1, max_stretch) with max_stretch inside the spread of the initial F (perturbed by 0.02),
    so that some particles break in the first substep, some later, and most never; odd seeds give a quarter of the
    particles another max_stretch and other Lame parameters of the projection (the per-particle plasticity layout)."""
    sc = _random_scene(seed)
    ps = sc["particles"]
    rng = np.random.default_rng(5000 + seed)
    ps.dp[:] = DruckerPrager.new(1e6, 0.25).as_array()
    ps.has_plasticity[:] = True
    ps.phase[:] = (1.0, 1.025)
    ps.has_phase[:] = True
    if seed % 2:
        q = rng.random(ps.n) < 0.25
        ps.phase[q, 1] = np.float32(1.04)
        ps.dp[q, 4:6] = DruckerPrager.new(3e5, 0.3).as_array()[4:6]
    return sc


@pytest.mark.parametrize("seed", [24, 25, 26, 27, 28, 29])
def test_random_breakable_plastic_scenes_match_oracle(hip_libs, oracle_libs, seed):
    """The fuzz of test_random_scenes_match_oracle over scenes whose particles break (max_stretch) and then flow
    (Drucker-Prager): the fracture switch and the projection against the oracle over many substeps and collider contacts."""
    sc = _breakable_scene(seed)
    got, st64 = _fuzz_parity(sc, 0)
    broke = (got.phase[:, 0] == 0.0).sum()
    assert 0 < broke < got.n, "some particles must break and some must not"


def _fuzz_parity(sc, chunk):
    dim = sc["particles"].dim
    k = 12
    data = step_chunks(sc, (chunk,) * (k // chunk) if chunk else (k,))
    st = run_oracle(sc, k, np.float32)
    st64 = run_oracle(sc, k, np.float64)
    cells, vm, dist, aff, closest = data.read_grid()
    oc, omv, odist, oaff, oclosest = st.grid_records()
    assert np.array_equal(cells, oc)
    report_margin("fuzz node affinity mismatch fraction", float((aff != oaff).mean()), FUZZ_NODE_MISMATCH)
    report_margin("fuzz node closest-id mismatch fraction", float((closest != oclosest).mean()), FUZZ_NODE_MISMATCH)
    assert (aff != oaff).mean() <= FUZZ_NODE_MISMATCH and (closest != oclosest).mean() <= FUZZ_NODE_MISMATCH
    got = data.read_particles()
    same = got.cdf_affinity == st.arr["cdf_affinity"]
    report_margin("fuzz particle affinity mismatch fraction", 1.0 - float(same.mean()), FUZZ_PART_MISMATCH)
    assert 1.0 - same.mean() <= FUZZ_PART_MISMATCH
    for f, tol in (("pos", 2e-5), ("vel", FUZZ_VEL_TOL)):
        err = rel_rms(getattr(got, f)[same], st64.arr[f][same])
        err32 = rel_rms(st.arr[f][same], st64.arr[f][same])
        report_margin(f"fuzz {f} rel rms vs fp64", err, tol, fp32_oracle_err=err32)
        assert err < tol, (f, err, err32)
    # the plastic and breakable state, and what the particle update leaves in F and C': phase exactly — a particle whose
    # fracture decision went the other way (s within round-off of max_stretch after 12 substeps of fp32 drift) is counted,
    # bounded like the affinity mismatches and left out of the floating-point fields, which then hold to the velocity bound
    # (F and C' are advanced from the same grid velocities)
    pmis = got.phase[same, 0] != st64.arr["phase"][same, 0]
    report_margin("fuzz phase mismatch fraction", float(pmis.mean()), FUZZ_PART_MISMATCH, count=int(pmis.sum()))
    assert pmis.mean() <= FUZZ_PART_MISMATCH
    assert np.array_equal(got.phase[:, 1], st64.arr["phase"][:, 1].astype(np.float32))
    keep = np.nonzero(same)[0][~pmis]
    for f in ("def_grad", "affine", "dp_state"):
        assert_close_to_truth(f"{f} (fuzz)", getattr(got, f)[keep], st.arr[f][keep], st64.arr[f][keep], FUZZ_VEL_TOL)
    if sc["colliders"]:
        st.update_world_mass_properties()
        worst = 0.0
        for gb, ob in zip(data.read_body_poses(), st.collider_states()):
            for key in ("rotation", "translation", "linvel", "angvel"):
                worst = max(worst, float(np.abs(np.asarray(gb[key]) - np.asarray(ob[key])).max()))
        report_margin("fuzz body state abs err", worst, FUZZ_BODY_ATOL)
        assert worst <= FUZZ_BODY_ATOL
    return got, st64


def test_long_near_collider_list_paths_match_the_separate_launches_and_the_oracle(hip_libs, monkeypatch):
    """Once wgs_sync has seen a long near-collider list, P2G runs its plain and its CPIC body in one launch (k_p2g_pair)
    and G2P sizes the list half of k_g2p_pair from it. A 262 k-particle corotated cube resting on the floor under a
    kinematic paddle (well over 8 listed blocks, two-way impulses on): the paired P2G ends bit-identical to the two separate
    launches (WGS_DEBUG P2G_TWO_LAUNCHES) — which path runs depends on when the host last synchronised, so the result must not —,
    the paired G2P agrees with the separate kernels (WGS_DEBUG G2P_TWO_LAUNCHES, a debug path; another compilation of the same
    source, one ulp apart), and the run matches the oracle."""
    sc = scenes.corotated_cube_with_paddle(n_side=64)

    def run():
        data = step_chunks(sc, (4, 4))                         # the host sees the list after the first call
        assert data.stats()["num_near_collider_blocks"] > 100  # a long list: the paired P2G launch is the one that ran
        return data.read_particles(), data.read_body_poses()
    pa, ba = run()
    with debug(monkeypatch, "P2G_TWO_LAUNCHES"):
        pb, bb = run()
        assert_same_bits(pa, pb, AFFINITY_FIELDS)
        assert_same_bodies(ba, bb, ("translation", "rotation", "linvel", "angvel"))
    with debug(monkeypatch, "G2P_TWO_LAUNCHES"):
        pc, _ = run()
        assert np.array_equal(pa.cdf_affinity, pc.cdf_affinity)
        for f in ("pos", "vel", "def_grad"):
            assert rel_rms(getattr(pc, f), getattr(pa, f)) < 1e-6, f
        st, st64 = run_oracle(sc, 8, np.float32), run_oracle(sc, 8, np.float64)
        same = pa.cdf_affinity == st.arr["cdf_affinity"]
        assert same.mean() > 0.999
        for f, tol in (("pos", 2e-6), ("vel", 2e-4)):
            err, err32 = rel_rms(getattr(pa, f)[same], st64.arr[f][same]), rel_rms(st.arr[f][same], st64.arr[f][same])
            assert err < max(tol, 10.0 * err32), (f, err, err32)


@pytest.mark.parametrize("seed", range(6))
def test_random_api_sequences_match_oracle(hip_libs, oracle_libs, seed):
    """Fuzz of the per-frame host writes (src_testbed/step.rs:79-119, ui.rs:91-104) interleaved with steps: random
    sequences of step / set_sim_params / set_body_velocities / full collider refresh, mirrored on the fp32 oracle."""
    import dataclasses
    sc = _random_scene(seed)
    if not sc["colliders"]:
        sc["colliders"] = [Collider.ball(1.5, tuple([5.0] * sc["particles"].dim))]
    dim = sc["particles"].dim
    rng = np.random.default_rng(7000 + seed)
    pipe, data = new_data(sc)
    st = oracle(dim, np.float32).new_state(sc["particles"], sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    cols = list(sc["colliders"])
    nc = len(cols)
    for _ in range(7):
        action = int(rng.integers(0, 4))
        if action == 0:
            p2 = SimulationParams(gravity=tuple(float(x) for x in rng.uniform(-10, 10, dim)), dt=float(rng.uniform(4e-4, 9e-4)))
            data.set_sim_params(p2); st.set_params(p2)
        elif action == 1:
            vel = (data.T.Velocity * nc)()
            for i in range(nc):
                lin = [float(x) for x in rng.uniform(-1, 1, 3)]
                ang = [float(x) for x in rng.uniform(-0.7, 0.7, 3)]
                if dim == 2:
                    lin[2] = 0.0; ang[1] = ang[2] = 0.0
                vel[i].linear = tuple(lin); vel[i].angular = tuple(ang)
                for kk in range(3):
                    st.cols[i].linvel[kk] = lin[kk]
                    st.cols[i].angvel[kk] = ang[kk]
            _ffi.check(data.lib, data.lib.wgs_set_body_velocities(data._h, vel, nc))
            st.moving = True
        elif action == 2:
            # full refresh from the host mirror: new poses (a small jump), velocities and mass properties
            new = []
            for c in cols:
                tr = tuple(float(x + dx) for x, dx in zip(c.translation, rng.uniform(-0.2, 0.2, dim)))
                new.append(dataclasses.replace(c, translation=tr, com=None if c.com is None else tr))
            cols = new
            data.set_colliders(cols); st.set_colliders(cols)
        n_sub = int(rng.integers(1, 6))              # (action 3 = just step)
        pipe.step(data, n_sub); st.step(n_sub)
    data.sync()
    got = data.read_particles()
    same = got.cdf_affinity == st.arr["cdf_affinity"]
    report_margin("api sequence affinity mismatch fraction", 1.0 - float(same.mean()), 0.005)
    report_margin("api sequence pos rel rms", rel_rms(got.pos[same], st.arr["pos"][same]), 2e-5)
    assert same.mean() > 0.995
    assert rel_rms(got.pos[same], st.arr["pos"][same]) < 2e-5


def test_body_setters_and_readback(hip_libs, oracle_libs):
    """wgs_set_body_velocities / wgs_set_collider_poses / wgs_set_body_mass_properties between steps, and the
    pose read-back of the testbed (src_testbed/step.rs:79-132): the device-integrated poses are not rolled back
    by a velocity write, a pose write moves the centre of mass with the body."""
    from golden_cases import dynamic_ball3d
    import dataclasses
    sc = dynamic_ball3d()
    pipe, data = new_data(sc)
    st = oracle(3, np.float64).new_state(sc["particles"], sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    pipe.step(data, 30); st.step(30)
    # velocity write only: poses keep what the device integrated
    cur = st.collider_states()
    data.lib.wgs_sync(data._h)
    vel = (data.T.Velocity * 2)()
    vel[0].linear = (0.1, -1.0, 0.0); vel[0].angular = (0.0, 0.5, 0.0)
    vel[1].linear = (0.0, 0.2, 0.0); vel[1].angular = (0.0, 0.0, -0.3)
    _ffi.check(data.lib, data.lib.wgs_set_body_velocities(data._h, vel, 2))
    for i in range(2):
        for k in range(3):
            st.cols[i].linvel[k] = vel[i].linear[k]
            st.cols[i].angvel[k] = vel[i].angular[k]
    pipe.step(data, 30); st.step(30)
    st.update_world_mass_properties()
    got, ref = data.read_body_poses(), st.collider_states()
    for i in range(2):
        for key in ("rotation", "translation", "linvel", "angvel", "com"):
            assert np.allclose(got[i][key], ref[i][key], rtol=0.0, atol=3e-4), (i, key, got[i][key], ref[i][key])
    assert np.abs(got[0]["translation"] - cur[0]["translation"]).max() < 0.2   # not rolled back to the initial pose
    # full refresh through the host mirror (poses + velocities + mass properties), body 0 made kinematic
    cols = [dataclasses.replace(sc["colliders"][0], translation=(21.5, 13.4, 22.0), linvel=(0.0, -0.5, 0.0),
                                inv_mass=(0.0,) * 3, inv_inertia_local=(0.0,) * 9), sc["colliders"][1]]
    data.set_colliders(cols); st.set_colliders(cols)
    pipe.step(data, 20); st.step(20)
    st.update_world_mass_properties()
    got, ref = data.read_body_poses(), st.collider_states()
    for i in range(2):
        for key in ("rotation", "translation", "linvel", "angvel", "com"):
            assert np.allclose(got[i][key], ref[i][key], rtol=0.0, atol=3e-4), (i, key, got[i][key], ref[i][key])
    assert abs(got[0]["linvel"][1] + 0.5) < 1e-6   # kinematic now: keeps its velocity, no gravity
    gp = data.read_particles()
    same = gp.cdf_affinity == st.arr["cdf_affinity"]
    assert same.mean() > 0.99
    assert rel_rms(gp.pos[same], st.arr["pos"][same]) < 1e-5


@pytest.mark.parametrize("name", ["tilted_box2d", "floor3d"])
def test_prep_vertex_buffer_modes(hip_libs, name):
    """Render hand-off: every RenderMode of src_testbed/prep_vertex_buffer{2,3}d.wgsl against its numpy
    restatement evaluated on the particle state read back from the same run."""
    from oracle import np_oracle
    make, k = _CASES[name]
    sc = make()
    data = run_gpu(sc, k)
    ps = data.read_particles()
    rng = np.random.default_rng(3)
    base = rng.uniform(0.0, 1.0, size=(ps.n, 4)).astype(np.float32)
    assert (ps.cdf_affinity != 0).any()
    for mode in range(6):
        got = data.prep_vertex_buffer(mode, base)
        ref = np_oracle.prep_instances(ps.pos, ps.vel, ps.def_grad, ps.cdf_normal, ps.cdf_dist, ps.cdf_affinity, mode,
                                       sc["cell_width"], sc["params"].dt, base)
        assert np.array_equal(got[:, :20], ref[:, :20].astype(np.float32)), mode       # F, position, base colour: copies
        tol = 2e-3 if mode == np_oracle.RENDER_VOLUME else 1e-6                         # (1 - S) / 0.005 amplifies 200 x
        assert np.allclose(got[:, 20:], ref[:, 20:], rtol=0.0, atol=tol), mode
    with pytest.raises(Exception):
        data.prep_vertex_buffer(17, base)


def test_c_abi_rejects_bad_arguments(hip_libs):
    """Error behaviour of the boundary: every entry point returns a status, nothing throws or aborts, and
    wgs_last_error explains."""
    import ctypes as C
    from golden_cases import mesh_floor3d
    from wgsparkl_amd.sampling import build_rigid_particles
    sc = mesh_floor3d()
    pipe, data = new_data(sc)
    lib, T, h = data.lib, data.T, data._h
    assert lib.wgs_step(None, h, 1, 0) != 0 and lib.wgs_step(pipe._h, None, 1, 0) != 0
    assert lib.wgs_set_sim_params(h, None) != 0
    poses = (T.Pose * 3)()
    assert lib.wgs_set_collider_poses(h, poses, None, 3) != 0            # more poses than colliders
    assert lib.wgs_set_body_velocities(h, None, 1) != 0
    assert lib.wgs_set_body_mass_properties(h, None, 2) != 0
    assert lib.wgs_read_body_poses(h, poses, None, None, 3) != 0
    assert lib.wgs_prep_vertex_buffer(h, 99, C.c_void_p(1)) != 0
    assert lib.wgs_set_plastic_state(h, None) != 0
    # rigid particles: ids must refer to existing vertices / colliders; a valid re-upload replaces the old buffers
    rb = build_rigid_particles(sc["colliders"], 3, sc["cell_width"])
    bad = dict(rb, ids=rb["ids"].copy())
    bad["ids"][0, 0] = len(rb["local_vtx"]) + 5
    with pytest.raises(Exception):
        data.set_rigid_particles(bad)
    bad = dict(rb, ids=rb["ids"].copy())
    bad["ids"][0, 3] = 7
    with pytest.raises(Exception):
        data.set_rigid_particles(bad)
    data.set_rigid_particles(rb)
    before = data.stats()["device_bytes"]
    for _ in range(3):
        data.set_rigid_particles(rb)
    assert data.stats()["device_bytes"] == before                        # no growth: the old buffers are released
    pipe.step(data, 5)
    data.sync()
    assert np.isfinite(data.read_positions()).all()
    many = [Collider.ball(1.0, (0.0, 0.0, 0.0))] * 17                    # the CPIC mask has 16 bits
    with pytest.raises(Exception):
        new_data(sc, colliders=many)


_GOLD = np.load(_os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "golden", "oracle_regression.npz"))


@pytest.mark.parametrize("name", sorted(_CASES))
def test_against_committed_golden_vectors(hip_libs, oracle_libs, name):
    make, k = _CASES[name]
    sc = make()
    dim = sc["particles"].dim
    data = run_gpu(sc, k)
    st32 = run_oracle(sc, k, np.float32)
    cpic = len(sc["colliders"]) > 0
    if cpic:
        truth = ({f: _GOLD[f"{name}/{f}"] for f in ("pos", "vel", "def_grad", "affine")}, _GOLD[f"{name}/grid_vm"])
        assert np.array_equal(st32.grid_records()[0], _GOLD[f"{name}/grid_cells"])
        assert np.array_equal(st32.grid_records()[3], _GOLD[f"{name}/grid_aff"])          # node affinity / sign bits: bit-exact
        compare_cpic(data, st32, None, dim, CPIC_GRID_V_TOL, CPIC_PART_TOL, min_same=0.995, h=sc["cell_width"], truth=truth)
    else:
        got = data.read_particles()
        for f in ("pos", "vel", "def_grad", "affine"):
            assert_close_to_truth(f, getattr(got, f), st32.arr[f], _GOLD[f"{name}/{f}"], PART_TOL)
        cells, vm, _, aff, _ = data.read_grid()
        assert np.array_equal(cells, _GOLD[f"{name}/grid_cells"])            # active nodes: bit-exact
        assert np.array_equal(aff, _GOLD[f"{name}/grid_aff"])
        o32 = grid_of(st32)[1]
        assert_close_to_truth("grid velocity", vm[:, :dim], o32[:, :dim], _GOLD[f"{name}/grid_vm"][:, :dim], GRID_V_TOL)
    if cpic:
        # rigid bodies, integrated on the device every substep (rigid_impulses.wgsl:95-136); the dynamic ones
        # are pushed by the particles (two-way coupling, p2g.wgsl:200-228). Absolute tolerance: positions are
        # O(10), velocities O(1), fixed-point impulses have a 1e-5 resolution.
        bodies = data.read_body_poses()
        for key in ("rotation", "translation", "linvel", "angvel"):
            got_b = np.stack([b[key] for b in bodies])
            assert np.allclose(got_b, _GOLD[f"{name}/body_{key}"], rtol=0.0, atol=3e-4), (key, got_b, _GOLD[f"{name}/body_{key}"])


def test_cpic_node_cdf_bit_exact(hip_libs, oracle_libs):
    """grid_update_cdf: distances within fp32 round-off, affinity bits and closest ids exact."""
    sc = _CASES["tilted_box2d"][0]()
    data = run_gpu(sc, 1)
    st = run_oracle(sc, 1, np.float32)
    cells, _, dist, aff, closest = data.read_grid()
    oc, _, odist, oaff, oclosest = st.grid_records()
    assert np.array_equal(cells, oc) and np.array_equal(aff, oaff) and np.array_equal(closest, oclosest)
    assert np.allclose(dist, odist, rtol=1e-5, atol=1e-5)


def test_long_run_stays_finite_with_floor(hip_libs):
    """C2-like scene with the floor cuboid, 400 substeps: nothing blows up, particles end above the floor."""
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=True)
    sc["particles"].pos[:, 1] -= 5.5
    data = run_gpu(sc, 400)
    got = data.read_particles()
    assert np.isfinite(got.pos).all() and np.isfinite(got.def_grad).all()
    assert got.pos[:, 1].min() > 1.5
    assert data.stats()["overflow"] == 0


def test_timestamps_and_stats(hip_libs):
    sc = cloud_scene(n=20000)
    data = run_gpu(sc, 4, timestamps=True)
    t = data.read_timings()
    assert t["grid sort"] > 0 and t["p2g"] > 0 and t["g2p"] > 0 and t["grid_update"] > 0
    assert t["particles_update"] == 0.0      # fused into "g2p"
    s = data.stats()
    assert s["num_particles"] == 20000 and s["substeps_done"] == 4 and s["num_active_blocks"] > 0


def test_queue_step_replay_api(hip_libs, oracle_libs):
    """The reference's call shape: queue_step once, encode N times (src_testbed/step.rs:122-128)."""
    sc = cloud_scene(n=5000, seed=13)
    pipe, data = new_data(sc, colliders=[])
    q = KernelInvocationQueue()
    pipe.queue_step(data, q, add_timestamps=False)
    for _ in range(3):
        q.encode()
    data.sync()
    ref = run_gpu(sc, 3).read_particles()
    got = data.read_particles()
    assert np.array_equal(got.pos, ref.pos) and np.array_equal(got.affine, ref.affine)


def test_set_sim_params_and_colliders(hip_libs, oracle_libs):
    """Per-frame host->device writes of the testbed (src_testbed/step.rs:79-119, ui.rs:91-104)."""
    sc = _CASES["tilted_box2d"][0]()
    pipe, data = new_data(sc)
    st = oracle(2, np.float32).new_state(sc["particles"], sc["params"], sc["colliders"], sc["cell_width"],
                                         sc["grid_capacity"], sc["model"])
    pipe.step(data, 5); st.step(5)
    p2 = SimulationParams(gravity=(1.0, -4.0), dt=sc["params"].dt * 0.5)
    cols = [Collider.cuboid((50.0, 1.0), (10.0, 1.3), rotation=(0.1,)),
            Collider.ball(2.0, (14.5, 6.0), linvel=(0.25, 0.1, 0.0), angvel=(-0.5,))]
    data.set_sim_params(p2); data.set_colliders(cols)
    st.set_params(p2); st.set_colliders(cols)
    pipe.step(data, 5); st.step(5)
    data.sync()
    got = data.read_particles()
    same = got.cdf_affinity == st.arr["cdf_affinity"]
    report_margin("setters affinity mismatch fraction", 1.0 - float(same.mean()), 0.005)
    report_margin("setters vel rel rms", rel_rms(got.vel[same], st.arr["vel"][same]), 1e-4)
    assert same.mean() > 0.995
    assert rel_rms(got.pos[same], st.arr["pos"][same]) < 1e-5
    assert rel_rms(got.vel[same], st.arr["vel"][same]) < 1e-4


def _flying_cube(speed, dt, capacity):
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=True, grid_capacity=capacity)
    ps = sc["particles"]
    rel = ps.pos - ps.pos.mean(0)
    ps.vel[:, 0] = speed + 1.5 * rel[:, 2]
    ps.vel[:, 1] = 0.6 * speed
    ps.vel[:, 2] = speed - 1.5 * rel[:, 0]
    sc["params"] = SimulationParams((0.0, 0.0, 0.0), dt)
    return sc


def test_oracle_parity_through_eviction_id_reuse_table_refresh_and_host_looks(hip_libs, oracle_libs):
    """The oracle rebuilds its grid from nothing every substep (grid.rs:30-207); the HIP path keeps table, ids and cell runs from substep to
    substep, evicts blocks nobody activated for 8 substeps, hands their ids out again, clears the marks out of the table when they crowd
    it (k_table_refresh) and sizes its launches by what the host saw at its last look. A 16^3 cube crossing the grid at half a cell per
    substep while spinning, 240 substeps in eight wgs_step calls with a wgs_sync after each: the block sets, the particles of every block
    and the per-block counts are the oracle's after EVERY call, the particle fields and the grid at the end are within the fp32 tolerances
    of the fp64 oracle — and the run did evict, did reuse ids and did refresh the table (wgs_stats), with no table rebuild after the first substep."""
    sc = _flying_cube(150.0, 1.0 / 300.0, 512)
    ps = sc["particles"]
    pipe, data = new_data(sc)
    st32 = oracle(3, np.float32).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], 4096, sc["model"])
    st64 = oracle(3, np.float64).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], 4096, sc["model"])
    handed_out = 0
    for call in range(8):
        pipe.step(data, 30)
        data.sync()
        st32.step(30)
        st64.step(30)
        assert not st32.overflow and not st64.overflow
        check_blocks(data, st32)
        s = data.stats()
        assert s["overflow"] == 0
        handed_out = max(handed_out, s["block_ids"])
    s = data.stats()
    assert s["table_rebuilds"] == 1 and s["grid_growths"] == 0, s        # the first substep only
    assert s["table_refreshes"] >= 1, s                                   # the marks did crowd the table, and were cleared
    assert s["block_ids_free"] > 0 or s["table_marks"] > 0, s             # blocks were evicted ...
    # ... and their ids handed out again: far more blocks were active over the run than ids exist
    assert handed_out <= s["grid_capacity"]
    # 240 substeps of a body that crosses a cell every other substep: the fp32 restatement of the reference's own arithmetic is 1.3e-5 off the
    # fp64 truth in the node masses by now (particles on the two sides of a rounding boundary) — the one-substep tolerances (1e-5 / 2e-5) do
    # not apply to a trajectory; 5e-5 here, with the fp32 oracle's own error reported beside the HIP path's (profiles/r06_parity_margins.json)
    LONG_TOL = 5e-5
    gv, ov = compare_grids(data.read_grid(), grid_of(st64))
    o32 = grid_of(st32)[1]
    assert_close_to_truth("grid velocity (240 substeps)", gv[:, :3], o32[:, :3], ov[:, :3], LONG_TOL)
    assert_close_to_truth("grid mass (240 substeps)", gv[:, 3], o32[:, 3], ov[:, 3], LONG_TOL)
    check_fields(data, st32, st64, tol=LONG_TOL)


def test_oracle_parity_of_the_reference_sand3_scene_across_host_looks(hip_libs, oracle_libs):
    """sand3 as shipped (crates/wgsparkl3d/examples/sand3.rs:28-113), three wgs_step calls of eight substeps with a wgs_sync after each:
    from the second call on the launches are shaped by what the host saw — the prologue waves of the P2G launch take the particle cdf of the
    listed blocks, the blocks within reach of the spinning cuboid share their node-cdf summaries (round 5's mechanisms, until now checked
    against debug shapes of the same library only). Blocks exact after every call; fields, node bits and the body's pose against the fp64
    oracle at the end."""
    sc = scenes.reference_sand3()
    ps = sc["particles"]
    pipe, data = new_data(sc)
    st32 = oracle(3, np.float32).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    st64 = oracle(3, np.float64).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    def block_of_particle(vid, first, num, ids):
        out = np.zeros((ps.n, 3), np.int64)
        for b in range(len(vid)):
            out[ids[first[b]:first[b] + num[b]]] = vid[b]
        return out
    for call in range(3):
        pipe.step(data, 8)
        data.sync()
        st32.step(8)
        st64.step(8)
        if call == 0:
            check_blocks(data, st32)
        else:
            # a trajectory, not a substep: after 16 / 24 substeps a grain that sits on a cell boundary to within fp32 round-off may be
            # associated with the neighbouring cell here and not in the fp32 restatement (both are the reference's arithmetic, in another
            # order). The active block SETS stay identical; the grains whose block differs are counted (at most one in 20 000) and
            # must sit within 1e-4 h of a cell boundary in the fp64 oracle
            vid, first, num, ids = data.read_blocks()
            ovid, ofirst, onum = st32.blocks()
            assert np.array_equal(vid, ovid), "active block sets differ"
            mine = block_of_particle(vid, first, num, ids)
            osorted = st32.g["sorted_ids"][:st32.n]
            theirs = block_of_particle(ovid, ofirst, onum, osorted)
            diff = np.where(np.any(mine != theirs, axis=1))[0]
            assert len(diff) <= ps.n // 20000, len(diff)
            if len(diff):
                x = st64.arr["pos"][diff] / sc["cell_width"]
                dist = np.abs(np.abs(x - np.floor(x)) - 0.5).min(axis=1)   # (assoc_cell = round(x / h) - 1 changes where frac(x / h) = 0.5)
                assert (dist < 1e-4).all(), dist
        assert data.stats()["num_near_collider_blocks"] > 0
    got, same = compare_cpic(data, st32, st64, 3, CPIC_GRID_V_TOL, 2e-4, min_same=0.995, fields=("pos", "vel", "def_grad"))
    assert (got.cdf_affinity != 0).sum() > 100, "the spinning cuboid must be felt"
    pose = data.read_body_poses()[5]
    want = st64.collider_states()[5]
    assert np.allclose(pose["rotation"], want["rotation"], atol=1e-5) and np.allclose(pose["translation"], want["translation"], atol=1e-5)


def test_one_call_of_two_thousand_substeps_keeps_its_table_in_order(hip_libs):
    """Upkeep INSIDE a call: the host takes its decisions (growth, rebuild, refresh of the table) between wgs_step calls; a caller that
    queues 2 000 substeps of a body flying across the grid in ONE call gives it no such moment. The call itself looks at its pinned
    counters every 64 substeps it has queued (capi_lifecycle.inc wgs_step: watch_counters + maintain_grid of host_grid.inc): the run ends without overflow, the table was refreshed on the way, and
    the result is the bits of the same 2 000 substeps queued a hundred at a time."""
    sc = _flying_cube(40.0, 1.0 / 300.0, 512)

    def run(chunks):
        data = step_chunks(sc, chunks)
        return data.read_particles(), data.stats()
    a, sa = run((2000,))
    b, sb = run((100,) * 20)
    assert sa["overflow"] == 0 and sb["overflow"] == 0, (sa, sb)
    assert sa["table_rebuilds"] == 1 and sb["table_rebuilds"] == 1, (sa["table_rebuilds"], sb["table_rebuilds"])
    assert sa["table_marks"] <= sa["grid_capacity"], sa      # (the marks never outnumber half the table's slots: 2 x capacity)
    assert_same_bits(a, b, BASE_FIELDS)
