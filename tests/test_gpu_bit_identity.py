"""-m gpu: results that must be THE SAME BITS — run to run, across launch shapes (WGS_DEBUG switches of the shipped library), with the sort's
binning inside the fused G2P or as a launch of its own, across a checkpoint / restart, with other data running on the device at the same time."""
import numpy as np
import pytest

from wgsparkl_amd import MpmData, _ffi, scenes
from wgsparkl_amd.models import (MODEL_COROTATED, MODEL_NEO_HOOKEAN, WALL_NONE, DruckerPrager, ElasticCoefficients, ParticlePhase)
from wgsparkl_amd.solver import Collider, ParticleSet, SimulationParams

from helpers import (AFFINITY_FIELDS, BASE_FIELDS, CDF_FIELDS, PLASTIC_FIELDS, assert_same_bits, assert_same_bodies, assert_same_grid, debug,
                     new_data, pipeline, rel_rms, restored_colliders, run_gpu, step_chunks)
from gpu_common import _random_scene, cloud_scene

pytestmark = pytest.mark.gpu


def test_determinism(hip_libs):
    sc = cloud_scene(n=30000, seed=11)
    a = run_gpu(sc, 5).read_particles()
    b = run_gpu(sc, 5).read_particles()
    assert_same_bits(a, b, BASE_FIELDS)


def test_uniform_material_mode_is_bit_identical(hip_libs, monkeypatch):
    """One material for all particles: the four per-particle constants (mass, V0, lambda, mu) become kernel arguments
    and F[8] rides in their place (layout.h, Dev::uniform) — 32 bytes per particle and substep less through HBM. Same
    arithmetic on the same values: bit-identical to the general layout (WGS_DEBUG NO_UNIFORM keeps that one), incl. the
    CPIC passes and Drucker-Prager, and the read-back shows the caller's constants."""
    for make in (lambda: scenes.neo_hookean_cube(n_side=20, with_floor=True), lambda: scenes.sand_column(nx=12, ny=20, nz=12, with_floor=True)):
        def run():
            sc = make()
            sc["particles"].pos[:, 1] -= 5.6
            sc["particles"].vel[:, 1] = -2.0
            data = run_gpu(sc, 30)
            return sc, data.read_particles(), data.read_grid()
        sc, a, ga = run()
        with debug(monkeypatch, "NO_UNIFORM"):
            _, b, gb = run()
        assert_same_bits(a, b, PLASTIC_FIELDS + ("mass", "init_volume", "lambda_", "mu"))
        assert np.array_equal(a.mass, sc["particles"].mass) and np.array_equal(a.mu, sc["particles"].mu)
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1])


@pytest.mark.parametrize("dim", [2, 3])
def test_uniform_plasticity_parameters_give_the_bits_of_the_general_layout(hip_libs, monkeypatch, dim):
    """Round 6 (layout.h Dev::uni_dp): when every particle carries the same Drucker-Prager h0..h3 the plastic fused G2P takes them
    as kernel arguments and leaves the DP0 quad alone (mode 1); when lambda, mu of the plasticity and max_stretch are shared as well,
    the per-particle plastic state is ONE quad (mode 2). Decided at creation, bitwise. Four clouds — everything shared with a
    breakable phase (mode 2), every other particle with its own plastic lambda / mu (mode 1), with its own max_stretch (mode 1),
    with its own h0 (general layout) — against WGS_DEBUG NO_UNIFORM (never a uniform mode): same bits, and the read-back shows the
    caller's parameters."""
    def cloud(kind):
        ps = scenes.random_cloud(2500, dim=dim, seed=11 + kind, extent=9.0, young=1e6, plasticity=DruckerPrager.new(1e6, 0.25),
                                 phase=ParticlePhase(1.0, 1.04) if kind != 3 else None)
        if kind == 1: ps.dp[::2, 4:6] *= np.float32(1.5)
        if kind == 2: ps.phase[::2, 1] = np.float32(1.08)
        if kind == 3: ps.dp[::2, 0] *= np.float32(0.9)
        return ps
    cols = [Collider.cuboid((50.0,) * dim, (5.0, -49.0) + ((5.0,) if dim == 3 else ()), **({} if dim == 3 else {"rotation": (0.0,)}))]
    for kind in range(4):
        def run():
            ps = cloud(kind)
            sc = dict(particles=ps, params=SimulationParams((0.0, -9.81, 0.0)[:dim], 5e-4), colliders=cols, cell_width=1.0, grid_capacity=4096, model=MODEL_COROTATED)
            return ps, run_gpu(sc, 30).read_particles()
        ps, a = run()
        with debug(monkeypatch, "NO_UNIFORM"):
            _, b = run()
        assert_same_bits(a, b, BASE_FIELDS + ("dp", "dp_state", "phase"), kind)
        assert np.array_equal(a.dp, ps.dp) and np.array_equal(a.phase[:, 1], ps.phase[:, 1]), kind
        assert (a.dp_state != np.array([1.0, 1.0, 0.0], np.float32)).any() and (kind == 3 or (a.phase[:, 0] == 0.0).any()), "the scene should have yielded and broken by now"


def test_g2p_launch_shapes_are_bit_identical(hip_libs, monkeypatch):
    """The fused G2P advances one chunk of 64 sorted particles per wave, or — from 1.5 M particles on, where the launch is
    bound by latency x occupancy — two, with both chunks' particle state requested up front (kernels_transfer.h). The
    large-scene shape forced on small scenes (WGS_DEBUG G2P_TWO_PASSES) must give the same bits: elastic with the floor
    (both bodies of the paired launch), plastic, 2D."""
    makes = (lambda: scenes.neo_hookean_cube(n_side=24, with_floor=True), lambda: scenes.sand_column(nx=12, ny=20, nz=12, with_floor=True),
             lambda: scenes.elastic_block_2d(nx=50, ny=40))
    for make in makes:
        def run():
            sc = make()
            sc["particles"].pos[:, 1] -= 5.6 if sc["particles"].dim == 3 else 4.6
            sc["particles"].vel[:, 0] = 1.5
            return run_gpu(sc, 25).read_particles()
        a = run()
        with debug(monkeypatch, "G2P_TWO_PASSES"):
            b = run()
        assert_same_bits(a, b, PLASTIC_FIELDS)


@pytest.mark.parametrize("seed", [1, 4, 9, 12])
def test_binning_inside_the_fused_g2p_is_bit_identical_to_the_rebin_launch(hip_libs, seed, monkeypatch):
    """Single-domain data: the fused G2P bins its own output for the next substep (new cell ids, block activation and totals,
    mover lists: g2p_body.inc, Dev::bin_next), and launch 1 of that substep's sort (k_rebin) is not launched. WGS_DEBUG
    REBIN_LAUNCH brings k_rebin back. The sort is only a permutation with a canonical order inside a cell, so 150 substeps — random
    colliders, particles flying through blocks, two table rebuilds, the calls cut at odd places with a wgs_sync between them —
    must end bit-identical, particles, grid, block set and counts; and both must have counted the same cell-changers."""
    monkeypatch.setenv("WGS_REHASH_PERIOD", "64")             # (developer override, same results; the default is 1024)

    def run():
        data = step_chunks(_random_scene(seed), (1, 7, 63, 2, 77))
        return data.read_particles(), data.read_grid(), data.read_blocks(), data.stats()
    a, ga, ka, sa = run()
    # (... and launch 2 of the sort puts the members of a dirty block's cells in order by ranking the newcomers among the stayers;
    # WGS_DEBUG CELL_INSERTION_SORT keeps the insertion sort that covers the cases the ranking does not: the same order)
    for switch in ("REBIN_LAUNCH", "CELL_INSERTION_SORT"):
        with debug(monkeypatch, switch):
            b, gb, kb, sb = run()
            assert_same_bits(a, b, PLASTIC_FIELDS, switch)
            assert_same_grid(ga, gb)
            assert np.array_equal(ka[0], kb[0]) and np.array_equal(ka[2], kb[2])   # (block set and counts; where a block sits in memory is up to the atomics)
            assert sa["cell_changers"] == sb["cell_changers"] and sa["cell_changers"] > 0
            assert sa["overflow"] == 0 and sb["overflow"] == 0


@pytest.mark.parametrize("which", ["dynamic_ball_and_polyline_2d", "cube_on_floor_3d", "sand_between_walls_3d"])
def test_data_stepped_concurrently_on_their_own_streams_stay_bit_identical(hip_libs, which):
    """Several wgs_data of one pipeline may run at the same time, each on its own stream (threading). The grid
    update waits INSIDE the P2G launch for slabs of other workgroups (kernels_transfer.h gu_waves) — a wait that must make
    progress, and hand over complete data, also while kernels of other data occupy the device. Four copies of a scene are
    stepped interleaved, no synchronisation between the calls (their kernels overlap), and must end with the same bits as a
    copy that ran alone; nobody may report a hand-over time-out."""
    def make():
        if which == "dynamic_ball_and_polyline_2d":
            sc = _random_scene(1)          # a dynamic ball pushed to its velocity cap, a kinematic cuboid, a moving polyline
        elif which == "cube_on_floor_3d":
            sc = scenes.neo_hookean_cube(n_side=40, with_floor=True)
            sc["particles"].pos[:, 1] -= 5.6
            sc["particles"].vel[:, 0] = 1.5
        else:
            sc = scenes.sand_column(nx=12, ny=20, nz=12, with_floor=True)
        return new_data(sc)
    pipe, alone = make()
    for k in (3, 17, 20):
        pipe.step(alone, k)
    alone.sync()
    ref = alone.read_particles()
    copies = [make()[1] for _ in range(4)]
    for k in (3, 17, 20):
        for _ in range(k):
            for c in copies:
                pipe.step(c, 1)
    for c in copies:
        c.sync()                 # (raises on ERRBIT_HANDOVER)
        assert_same_bits(c.read_particles(), ref, PLASTIC_FIELDS)
        assert c.stats()["overflow"] == 0


def test_grid_update_inside_the_p2g_launch_is_bit_identical_to_its_own_launch(hip_libs, monkeypatch):
    """Single-domain simulations run the grid update as waves of the (last) P2G launch: P2G hands its slabs over
    inside the launch (write-through stores, one word per block), the waves gather past their XCD's L2
    (kernels_transfer.h gu_waves). WGS_DEBUG GU_OWN_LAUNCH brings the launch of its own back: same sums in the same order, so
    the same bits — no colliders (one P2G launch), a floor in contact (two launches, then the paired one after the
    host has seen the list), plastic between walls, 2D; particles AND the grid (nodes, slabs' velocities feed the G2P)."""
    makes = (lambda: scenes.neo_hookean_cube(n_side=24), lambda: scenes.neo_hookean_cube(n_side=40, with_floor=True),
             lambda: scenes.sand_column(nx=12, ny=20, nz=12, with_floor=True), lambda: scenes.elastic_block_2d(nx=50, ny=40),
             lambda: scenes.corotated_cube_with_paddle(n_side=32))   # (two-way coupling: node impulses gathered by the same waves)
    for make in makes:
        def run():
            sc = make()
            if sc["colliders"] and len(sc["colliders"]) == 1:
                sc["particles"].pos[:, 1] -= 5.6 if sc["particles"].dim == 3 else 4.6
            sc["particles"].vel[:, 0] = 1.5
            pipe, data = new_data(sc)
            pipe.step(data, 12)
            data.sync()          # (a long near-collider list seen here switches P2G to its paired launch)
            pipe.step(data, 13)
            return data.read_particles(), data.read_grid(), data.read_body_poses()
        a, ga, ba = run()
        with debug(monkeypatch, "GU_OWN_LAUNCH"):
            b, gb, bb = run()
        assert_same_bits(a, b, PLASTIC_FIELDS)
        assert_same_grid(ga, gb)
        assert_same_bodies(ba, bb, ("translation", "rotation", "linvel", "angvel"))
        if len(ba) > 1:      # moving bodies: integrate_bodies rides in the next substep's first sort launch (524288: a launch of its own)
            with debug(monkeypatch, "BODIES_OWN_LAUNCH"):
                c, _, bc = run()
            assert_same_bits(a, c, AFFINITY_FIELDS)
            assert_same_bodies(ba, bc, ("translation", "rotation", "linvel", "angvel"))


@pytest.mark.parametrize("seed", [0, 3, 8])
def test_steady_state_rebinning_is_bit_identical_to_full_binning(hip_libs, seed, monkeypatch):
    """k_rebin (re-binning relative to the previous substep's blocks) against the general k_bin forced on every
    substep (WGS_DEBUG NO_REBIN, read when the data is created): the sort is only a permutation, so 150 substeps —
    across two table rebuilds — must end bit-identical."""
    sc = _random_scene(seed)
    k = 150
    monkeypatch.setenv("WGS_REHASH_PERIOD", "64")             # (developer override, same results; the default is 1024)
    a = run_gpu(sc, k).read_particles()
    with debug(monkeypatch, "NO_REBIN"):
        b = run_gpu(sc, k).read_particles()
        assert_same_bits(a, b, PLASTIC_FIELDS)


def test_plastic_pair_register_budgets_are_bit_identical(hip_libs, monkeypatch):
    """Drucker-Prager sand between a floor and four walls, half of the blocks near a collider: after the first wgs_sync
    the fused G2P runs the variant compiled for 2 waves per SIMD (no spills in the CPIC body). Same source, another
    register budget: the results must be the bits of the 3-waves variant (WGS_DEBUG NO_G2P_DENSE keeps that one), because
    which of the two runs depends on when the host synchronised."""
    sc = scenes.sand_column(nx=40, ny=60, nz=40, with_walls=True)
    sc["particles"].pos[:, 1] -= 5.8

    def run():
        pipe, data = new_data(sc)
        pipe.step(data, 4)
        data.sync()
        st = data.stats()
        assert st["num_near_collider_blocks"] * 2 >= st["num_active_blocks"]     # the switch condition of host_substep.inc plan_g2p
        pipe.step(data, 8)
        data.sync()
        return data.read_particles()
    a = run()
    with debug(monkeypatch, "NO_G2P_DENSE"):
        b = run()
        assert_same_bits(a, b, PLASTIC_FIELDS)
        assert np.isfinite(a.pos).all() and len(sc["colliders"]) == 5
    # the one-way P2G pair has two register budgets too (chosen from the particle count and the list length): force the
    # small one by making the scene "large" is not possible at this size, so compare the large budget (this scene's
    # choice) with the separate launches, and the small budget at a size that selects it below
    with debug(monkeypatch, "P2G_TWO_LAUNCHES"):
        c = run()
        assert_same_bits(a, c, PLASTIC_FIELDS)
        for c in range(5):
            assert ((a.cdf_affinity >> c) & 1).sum() > 100, c


def test_large_one_way_scenes_do_not_depend_on_when_the_host_synchronised(hip_libs, monkeypatch):
    """From 600 k particles on, one-way collider simulations always run the paired P2G launch with the CPIC body cut to
    168 VGPRs — a budget that differs from the unconstrained one in the last bit here and there, so it must not follow
    the near-collider list the host last saw. 640 k neo-Hookean particles lying on the floor: eight substeps in one call
    and the same eight with a wgs_sync after the third end bit-identical; the unconstrained budget (WGS_DEBUG NO_P2G_SMALL_BUDGET)
    agrees to round-off."""
    sc = scenes.neo_hookean_cube(n_side=86, with_floor=True)
    sc["particles"].pos[:, 1] -= 5.7
    assert sc["particles"].n >= 600_000

    def run(chunks):
        data = step_chunks(sc, chunks)
        assert data.stats()["num_near_collider_blocks"] >= 8
        return data.read_particles()
    a, b = run((8,)), run((3, 5))
    assert_same_bits(a, b, AFFINITY_FIELDS)
    with debug(monkeypatch, "NO_P2G_SMALL_BUDGET"):
        c = run((3, 5))
        assert np.array_equal(a.cdf_affinity, c.cdf_affinity)
        for f in ("pos", "vel", "def_grad"):
            assert rel_rms(getattr(c, f), getattr(a, f)) < 1e-6, f


@pytest.mark.parametrize("seed", [1, 2, 6, 8])
def test_checkpoint_restart_random_scenes(hip_libs, seed):
    """Bit-exact restart on the fuzz scenes: dynamic and kinematic bodies, mesh colliders, plasticity."""
    sc = _random_scene(seed)
    dim = sc["particles"].dim
    pipe, full = new_data(sc)
    pipe.step(full, 20)
    _, part = new_data(sc)
    pipe.step(part, 9)
    snap, bodies = part.read_particles(), part.read_body_poses()
    _, rest = new_data(sc, particles=snap, colliders=restored_colliders(sc["colliders"], bodies, dim))
    rest.set_plastic_state(snap.dp_state)
    pipe.step(rest, 11)
    a, b = full.read_particles(), rest.read_particles()
    exact = dim == 3     # 2D poses are handed over as an angle: cos / sin round-trip costs an ulp
    if exact or not sc["colliders"]:
        assert_same_bits(a, b, PLASTIC_FIELDS)
    else:
        for f in BASE_FIELDS + ("dp_state",):
            assert rel_rms(getattr(b, f), getattr(a, f)) < 1e-4, f


def test_checkpoint_restart_is_bit_exact(hip_libs):
    """read_particles (+ plastic state, + body poses) -> MpmData.new -> set_plastic_state continues the
    run bit-for-bit (every reduction is in canonical particle order, whatever the storage order)."""
    ps = scenes.random_cloud(3000, dim=3, seed=5, extent=10.0, young=1e6, plasticity=DruckerPrager.new(1e6, 0.25), phase=None)
    ps.pos[:, 1] += 3.0
    cols = [Collider.cuboid((50.0, 1.0, 50.0), (8.0, 1.0, 8.0)),
            Collider.ball(1.5, (8.0, 12.0, 8.0), linvel=(0.0, -1.0, 0.0), angvel=(0.0, 0.0, 0.5))]
    sc = dict(particles=ps, params=SimulationParams((0.0, -9.81, 0.0), 5e-4), colliders=cols, cell_width=1.0, grid_capacity=4096, model=MODEL_COROTATED)
    pipe, full = new_data(sc)
    pipe.step(full, 24)
    _, part = new_data(sc)
    pipe.step(part, 12)
    snap, bodies = part.read_particles(), part.read_body_poses()
    assert (snap.dp_state != np.array([1.0, 1.0, 0.0], np.float32)).any(), "scene should have yielded by now"
    _, rest = new_data(sc, particles=snap, colliders=restored_colliders(cols, bodies, 3))
    rest.set_plastic_state(snap.dp_state)
    pipe.step(rest, 12)
    assert_same_bits(full.read_particles(), rest.read_particles(), CDF_FIELDS + ("phase",))
    assert_same_bodies(full.read_body_poses(), rest.read_body_poses())


def test_checkpoint_restart_with_a_rotated_fixed_collider_next_to_a_moving_one(hip_libs):
    """A fixed collider is BIT-static whatever else moves (kernels_bodies.h bodies_integrate_one skips the identity
    integration of a body at rest): node cdfs cached out of reach of the moving colliders (Dev::cdf_moving) stay those a
    restarted run computes, and the pose a run reads back after any number of substeps is the one it was given."""
    ps = scenes.random_cloud(4000, dim=3, seed=11, extent=10.0, young=1e6)
    ps.pos[:, 1] += 4.0
    q = np.array([0.13, -0.31, 0.22, 0.91])
    q = tuple((q / np.linalg.norm(q)).astype(np.float32).astype(float))
    cols = [Collider.cuboid((50.0, 1.0, 50.0), (8.0, 0.5, 8.0), rotation=q),
            Collider.ball(1.5, (8.0, 13.0, 8.0), linvel=(0.0, -2.0, 0.0), angvel=(0.3, 0.0, 0.5))]
    sc = dict(particles=ps, params=SimulationParams((0.0, -9.81, 0.0), 5e-4), colliders=cols, cell_width=1.0, grid_capacity=4096, model=MODEL_NEO_HOOKEAN)
    pipe, full = new_data(sc)
    pose0 = full.read_body_poses()[0]
    pipe.step(full, 30)
    _, part = new_data(sc)
    pipe.step(part, 13)
    snap, bodies = part.read_particles(), part.read_body_poses()
    for key in ("translation", "rotation"):
        assert np.array_equal(bodies[0][key], pose0[key]), f"the fixed collider's {key} changed bits"
    _, rest = new_data(sc, particles=snap, colliders=restored_colliders(cols, bodies, 3))
    rest.set_plastic_state(snap.dp_state)   # (phase None: the reference's default Drucker-Prager, quirk B1 — the scene is plastic)
    pipe.step(rest, 17)
    assert_same_bits(full.read_particles(), rest.read_particles(), AFFINITY_FIELDS + ("cdf_normal", "cdf_dist"))
    assert_same_grid(full.read_grid(), rest.read_grid())


@pytest.mark.parametrize("plastic", [False, True])
def test_a_body_crossing_the_grid_evicts_blocks_and_stays_bit_identical_to_the_rebuild_path(hip_libs, plastic, monkeypatch):
    """A cube flies through the grid and spins for 2 000 substeps: it leaves a trail of blocks nobody activates any more. Launch 2 of
    the sort evicts them (their table slots are marked, their ids reused: kernels_sort.h regroup_block) — no table rebuild but the
    periodic ones; with WGS_DEBUG NO_EVICTION nothing is evicted and the table is rebuilt whenever three quarters of the ids are handed out.
    The sort is only a permutation: the same bits either way, and the evicting run rebuilds less often."""
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=True, grid_capacity=512)   # (~125-200 blocks at a time: the grid never grows; 384 ids run out every few hundred substeps)
    ps = sc["particles"]
    if plastic:   # (the variants with the plasticity / fracture branch bin in launch 1 of the sort, k_rebin, not in the fused G2P; a
        # breakable phase that never breaks selects them and leaves the cube in one piece)
        ps = ParticleSet.uniform(sc["particles"].pos, 0.25, 2700.0, ElasticCoefficients.from_young_modulus(1.0e7, 0.2),
                                 phase=ParticlePhase(1.0, 1.0e6))
    rel = ps.pos - ps.pos.mean(0)
    ps.vel[:, 0] = 40.0 + 1.5 * rel[:, 2]
    ps.vel[:, 1] = 25.0
    ps.vel[:, 2] = 40.0 - 1.5 * rel[:, 0]
    sc["params"] = SimulationParams((0.0, 0.0, 0.0), 1.0 / 300.0)   # (270 cells along x and z, 170 along y in 2 000 substeps)
    monkeypatch.setenv("WGS_REHASH_PERIOD", "100000")   # (developer override, same results: no periodic rebuild inside the run)
    def run():
        data = step_chunks(new_data(sc, particles=ps)[1], (100,) * 20)
        return data.read_particles(), data.stats()
    a, sa = run()
    with debug(monkeypatch, "NO_EVICTION"):
        b, sb = run()
        assert_same_bits(a, b, BASE_FIELDS + ("dp_state",))
        assert sa["overflow"] == 0 and sb["overflow"] == 0
        assert sa["table_rebuilds"] < sb["table_rebuilds"], (sa["table_rebuilds"], sb["table_rebuilds"])
        assert sa["table_rebuilds"] <= 1 + sa["grid_growths"]     # the first substep (+ one per growth of the grid: none expected)


@pytest.mark.parametrize("scene", ["sand3", "paddle"])
def test_node_cdf_summaries_shared_between_blocks_give_the_bits_of_whole_tile_evaluation(hip_libs, scene, monkeypatch):
    """Where a collider moves, launch 2 of the sort evaluates every block's OWN nodes against the colliders and lets the block's
    neighbours know which of them have an affinity (Dev::block_cdf_summ, kernels_sort.h) instead of evaluating the (BW+2)^3 tile of
    every block — each node up to eight times. The class of a block (listed for the CPIC bodies or not) and everything downstream must
    be what the whole-tile evaluation gives (WGS_DEBUG NO_CDF_SUMM), also when no word is ever waited for (WGS_DEBUG CDF_SUMM_NO_WAIT: every neighbour whose
    word is late is evaluated locally — the path taken when a neighbour's wave is not resident)."""
    if scene == "sand3":
        sc = scenes.reference_sand3()
        steps = 150
    else:   # a box swept through a block of elastic material resting on the floor: the set of blocks in reach changes every substep
        sc = scenes.neo_hookean_cube(n_side=40, with_floor=True)
        sc["particles"].pos[:, 1] -= sc["particles"].pos[:, 1].min() - 2.5 * sc["cell_width"]
        lo, hi = sc["particles"].pos.min(0), sc["particles"].pos.max(0)
        paddle = Collider.cuboid((0.6, 2.0, 6.0), translation=(float(lo[0]) - 1.0, float(0.5 * (lo[1] + hi[1])), float(0.5 * (lo[2] + hi[2]))),
                                 linvel=(30.0, 0.0, 0.0))
        sc["colliders"] = list(sc["colliders"]) + [paddle]
        steps = 200
    def run():
        data = run_gpu(sc, steps)
        return data.read_particles(), data.stats()
    a, sa = run()
    assert sa["overflow"] == 0
    assert np.any(a.cdf_affinity != 0)   # (somebody is within reach of a collider)
    for dbg in ("NO_CDF_SUMM", "CDF_SUMM_NO_WAIT"):
        with debug(monkeypatch, dbg):
            b, sb = run()
            assert_same_bits(a, b, CDF_FIELDS, dbg)


@pytest.mark.parametrize("scene", ["sand3", "paddle", "sand2"])
def test_particle_cdf_by_prologue_waves_of_the_p2g_launch_gives_the_bits_of_the_in_workgroup_prologue(hip_libs, scene, monkeypatch):
    """With a short near-collider list (as of the host's last look) the paired P2G launch computes the particle cdf of the listed
    blocks in prologue WAVES, one per visit-list entry, ahead of its workgroups, and hands the quads over inside the launch
    (written through, counted per block, fetched past the L2: kernels_transfer.h pcdf_waves) instead of in three to six rounds inside
    each block's CPIC workgroup. Same particles, same arithmetic: the same bits as with WGS_DEBUG NO_PCDF_WAVES (never prologue waves), substep
    after substep across host looks."""
    if scene == "sand3":
        sc = scenes.reference_sand3()
    elif scene == "sand2":
        sc = scenes.reference_sand2()
    else:
        sc = scenes.corotated_cube_with_paddle(n_side=32)
    def run():
        data = step_chunks(sc, (10,) * 12)   # (the host looks at the lists after each: the next call sizes its launches from what it saw)
        st = data.stats()
        return data.read_particles(), st, (data.read_body_poses() if sc["colliders"] else None)
    a, sa, ba = run()
    assert sa["overflow"] == 0 and sa["num_near_collider_blocks"] > 0
    # 4: never prologue waves; 8: prologue workgroups sized for an empty list whatever the host saw — the launch then decides from the
    # lists of the substep itself (too long for so few waves: the blocks' workgroups do the work; short enough: the waves do)
    for dbg in ("NO_PCDF_WAVES", "PCDF_WAVES_UNSIZED"):
        with debug(monkeypatch, dbg):
            b, sb, bb = run()
            assert_same_bits(a, b, CDF_FIELDS, dbg)
            if ba is not None:
                assert_same_bodies(ba, bb)


@pytest.mark.parametrize("scene", ["at_rest", "landed", "flying"])
def test_direct_runs_of_unchanged_blocks_give_the_bits_of_the_gather_through_the_permutation(hip_libs, scene, monkeypatch):
    """A block whose run is its previous run member for member (nobody moved, nobody arrived) is handed to the plain body of P2G with
    its cells' runs in the buffer's own coordinates: the particles are read where they are, without the gather through `perm`
    (layout.h CELL_DIRECT; one dependent round trip less per block). The same particles in the same order: the same bits as with
    WGS_DEBUG NO_DIRECT_RUNS (every block through the permutation) — a cube in free fall (every block direct), the cube landing on the floor
    (direct and gathered blocks side by side, listed blocks beside them) and the cube crossing the grid and spinning (hardly any direct
    block; blocks becoming direct and dirty again), with a host look in between."""
    sc = scenes.neo_hookean_cube(n_side=86, with_floor=True)
    ps = sc["particles"]
    nsub = 12
    if scene == "landed":
        ps.pos[:, 1] -= 5.7
        ps.vel[:, 1] = -3.0
        nsub = 24
    elif scene == "flying":
        r = ps.pos - ps.pos.mean(0)
        ps.vel[:] = (np.array([4.0, 2.5, 3.0]) + np.cross(np.array([0.0, 0.3, 0.1]), r)).astype(np.float32)
        nsub = 60

    def run():
        data = step_chunks(sc, (nsub // 2, nsub - nsub // 2))
        st = data.stats()
        assert st["overflow"] == 0
        return data.read_particles(), data.read_grid(), st
    a, ga, sta = run()
    with debug(monkeypatch, "NO_DIRECT_RUNS"):
        b, gb, stb = run()
        assert_same_bits(a, b, AFFINITY_FIELDS)
        assert_same_grid(ga, gb)
        if scene == "flying":
            assert sta["cell_changers"] > 0   # (the scene does move: blocks are dirty)


def test_large_two_way_scenes_with_the_near_collider_launch_first_give_the_bits_of_the_other_order(hip_libs, monkeypatch):
    """Large simulations with a body that moves (>= 600 k particles: BASELINE.json configs[3]) run P2G as two launches; since round 6 the
    near-collider launch goes FIRST and the grid update rides behind the plain launch (at the plain body's occupancy instead of the two-way
    body's). Same slabs, same gather: the bits of the plain-launch-first order (WGS_DEBUG PLAIN_P2G_FIRST), also across a host look."""
    sc = scenes.config_scene("c4", n_side=86)
    assert sc["particles"].n >= 600_000

    def run():
        data = step_chunks(sc, (30, 30))
        st = data.stats()
        assert st["overflow"] == 0 and st["num_near_collider_blocks"] > 0
        return data.read_particles(), data.read_grid(), data.read_body_poses()
    a, ga, pa = run()
    with debug(monkeypatch, "PLAIN_P2G_FIRST"):
        b, gb, pb = run()
        assert_same_bits(a, b, AFFINITY_FIELDS)
        assert_same_grid(ga, gb)
        assert_same_bodies(pa, pb, ("rotation", "translation", "linvel", "angvel"))


@pytest.mark.parametrize("dim", [3, 2])
def test_from_scene_builds_what_new_builds(hip_libs, dim):
    """MpmData.from_scene is MpmData.new with the scene's entries: the same small scene (a floor under it) created both ways and advanced
    two substeps ends with the same bits in the particles, the grid and the body poses, and the same counters; a keyword replaces the
    scene's entry. Then a scene with every optional key (a small block_in_fluid between grid walls, Tait exponent 5): MpmData.new and
    the three setters by hand against from_scene — the same digest, particles, per-particle models and walls after two substeps; and
    `models=None` builds it without its table."""
    pipe = pipeline(dim)

    def spelled(sc):
        return MpmData.new(pipe, sc["params"], sc["particles"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])

    sc = scenes.neo_hookean_cube(n_side=8, with_floor=True) if dim == 3 else scenes.elastic_block_2d(22, 22)
    assert sc["particles"].n == (512 if dim == 3 else 484)
    a, b = step_chunks(spelled(sc), (2,)), step_chunks(MpmData.from_scene(pipe, sc), (2,))
    assert_same_bits(a.read_particles(), b.read_particles(), CDF_FIELDS)
    assert_same_grid(a.read_grid(), b.read_grid())
    assert a.n_colliders == b.n_colliders == len(sc["colliders"])
    assert_same_bodies(a.read_body_poses(), b.read_body_poses())
    assert a.stats() == b.stats()
    assert MpmData.from_scene(pipe, sc, colliders=[]).n_colliders == 0

    sc = scenes.block_in_fluid(dim, tank=(12, 8, 8) if dim == 3 else (24, 12), block=4, gap=0.1, drop_speed=6.0, walls="grid", gamma=5.0)
    assert sc["fluid_gamma"] == 5.0 and sc["walls"] is not None and len(np.unique(sc["models"])) == 2 and sc["particles"].n <= 10_000
    a = spelled(sc)
    a.set_fluid_eos(sc["fluid_gamma"])
    a.set_particle_models(sc["models"])
    a.set_domain_walls(sc["walls"])
    a, b = step_chunks(a, (2,)), step_chunks(MpmData.from_scene(pipe, sc), (2,))
    assert a.diagnostics(_ffi.DIAG_DIGEST).digest == b.diagnostics(_ffi.DIAG_DIGEST).digest
    assert_same_bits(a.read_particles(), b.read_particles(), CDF_FIELDS)
    assert np.array_equal(a.read_particle_models(), b.read_particle_models()) and np.array_equal(b.read_particle_models(), sc["models"])
    assert a.domain_walls() == b.domain_walls() and any(w.type != WALL_NONE for w in b.domain_walls())
    assert np.all(MpmData.from_scene(pipe, sc, models=None).read_particle_models() == sc["model"])
