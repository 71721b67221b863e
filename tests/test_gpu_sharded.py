"""-m gpu: one scene cut into x-slabs (kernels_shard.h, host_sharded.inc, capi_sharded.inc) on one GPU — lockstep groups with device copies as the transport, one
rank over a real RCCL communicator as its own neighbours — against the single-domain run of the same scene."""
import numpy as np
import pytest

from wgsparkl_amd import scenes
from wgsparkl_amd.models import ParticlePhase
from wgsparkl_amd.sharded import by_id, join_slabs, lockstep_slabs
from wgsparkl_amd.solver import Collider, SimulationParams

from helpers import assert_joined_close, debug, max_abs, new_data, pipeline, rel_rms, report_margin, run_gpu
from gpu_common import FUZZ_BODY_ATOL

from golden_cases import CASES as _CASES

pytestmark = pytest.mark.gpu


def test_bench_decomposition_eight_ranks_on_one_gpu(hip_libs):
    """The N = 8 workload of bench.py (one elastic bar cut into 8 x-slabs, every rank generating only its own slab,
    the floor collider, bench.py's buffer capacities) advanced as a lockstep group on one GPU — wgs_sharded_step_lockstep:
    the per-phase code of wgs_sharded_step with device-to-device copies as the transport —: same particles as the
    single-domain run of the whole bar, none lost."""
    from wgsparkl_amd.sharded import NativeShard, native_lockstep, uniform_material_of
    world, n_side, k = 8, 24, 40
    full = scenes.neo_hookean_bar(n_side=n_side, world=world, rank=None)
    vx = lambda gid: (8.0 + 3.0 * np.sin(0.37 * gid.astype(np.float64))).astype(np.float32)   # particles cross the faces
    full["particles"].vel[:, 0] = vx(full["global_ids"])
    pipe, ref_data = new_data(full, grid_capacity=full["grid_capacity"] * 4)
    pipe.step(ref_data, k)
    ref = ref_data.read_particles()
    shards, total = [], 0
    for rank in range(world):
        sc = scenes.neo_hookean_bar(n_side=n_side, world=world, rank=rank)
        ps = sc["particles"]
        ps.vel[:, 0] = vx(sc["global_ids"])
        total += ps.n
        shards.append(NativeShard.from_scene(pipe, sc, rank, particle_capacity=int(ps.n * 1.25) + 4096, uniform_material=uniform_material_of(ps),
                                             halo_capacity_records=2 * ((n_side // 8 + 3) ** 2 + 32), migrant_capacity=512))
    assert total == full["global_particles"] == full["particles"].n
    n0 = [s.num_particles() for s in shards]
    native_lockstep(pipe, shards, k)
    for s in shards:
        s.sync()                                             # would report a message / capacity overflow
    joined = join_slabs([s.export() for s in shards], full["global_ids"])
    assert joined.counts != n0, "particles must have crossed the faces"
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 1e-5)), "bench decomposition, 8 slabs, {f}", ref_order=np.argsort(full["global_ids"]))


@pytest.mark.parametrize("seed", range(6))
def test_random_scenes_sharded_match_single_domain(hip_libs, seed):
    """Fuzz-style check of the decomposition: random clouds (stretched along x so that every slab is a few blocks wide)
    with kinematic analytic colliders, cut into 2-4 slabs, advanced as a lockstep group (wgs_sharded_step_lockstep),
    against the single-domain run on the same GPU."""
    from wgsparkl_amd.sharded import native_lockstep
    rng = np.random.default_rng(500 + seed)
    dim = 3 if seed % 2 == 0 else 2
    world = int(rng.integers(2, 5))
    stretch = 3.0 if dim == 3 else 5.0
    ps = scenes.random_cloud(4000, dim=dim, seed=300 + seed, extent=22.0, young=1e6, phase=ParticlePhase(1.0, -1.0),
                             vel_scale=2.5, perturb_F=0.02, perturb_C=0.2)
    ps.pos[:, 0] *= np.float32(stretch)
    ps.vel[:, 0] += np.float32(rng.uniform(-6.0, 6.0))      # a drift: particles cross the cuts
    cols = []
    for _ in range(int(rng.integers(0, 3))):
        pos = [float(x) for x in rng.uniform(2.0, 20.0, dim)]
        pos[0] *= stretch
        kw = dict(linvel=tuple(float(x) for x in rng.uniform(-1.0, 1.0, 3)),
                  angvel=tuple(float(x) for x in rng.uniform(-0.5, 0.5, 3 if dim == 3 else 1)))
        cols.append(Collider.ball(float(rng.uniform(1.0, 3.0)), tuple(pos), **kw) if rng.random() < 0.5 else
                    Collider.cuboid(tuple(float(x) for x in rng.uniform(1.0, 4.0, dim)), tuple(pos), **kw))
    g = (0.0, -9.81, 0.0)[:dim]
    sc = dict(particles=ps, params=SimulationParams(gravity=g, dt=8e-4), colliders=cols, cell_width=1.0,
              grid_capacity=4096, model=int(rng.integers(0, 2)))
    k = 30
    ref = run_gpu(sc, k).read_particles()
    pipe = pipeline(dim)
    shards, part = lockstep_slabs(pipe, sc, world)
    assert part.min_interior_width() >= 3
    n0 = [s.num_particles() for s in shards]
    native_lockstep(pipe, shards, k)
    for s in shards:
        s.sync()
    joined = join_slabs([s.export() for s in shards], np.arange(ps.n))
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 2e-4)), "sharded fuzz {f}", migrated=bool(joined.counts != n0))


def test_sharded_run_with_kinematic_collider(hip_libs):
    """configs[3]'s decomposition on one GPU at a small size: the corotated bar on the floor, cut into 4 slabs, and the
    kinematic rotating cuboid at its end, which every rank integrates identically; particles, CPIC state and the body
    pose match the single-domain run (the bar slides towards the cuboid, so particles cross the cuts)."""
    from wgsparkl_amd.sharded import NativeShard, native_lockstep, uniform_material_of
    k, world, n = 30, 4, 24

    def c4(rank):
        sc = scenes.config_scene("c4", world, rank, "weak", n_side=n)
        sc["particles"].vel[:, 0] = (16.0 + 2.0 * np.sin(0.37 * sc["global_ids"].astype(np.float64))).astype(np.float32)
        return sc
    full = c4(None)
    single = run_gpu(full, k)
    ref, ref_body = single.read_particles(), single.read_body_poses()
    assert ((ref.cdf_affinity & 2) != 0).sum() > 100       # the paddle does touch the bar
    pipe = pipeline(3)
    shards = []
    for r in range(world):
        sc = c4(r)
        shards.append(NativeShard.from_scene(pipe, sc, r, particle_capacity=full["particles"].n, uniform_material=uniform_material_of(sc["particles"]),
                                             halo_capacity_records=512, migrant_capacity=2048))
    n0 = [s.num_particles() for s in shards]
    native_lockstep(pipe, shards, k)
    for s in shards:
        s.sync()
    joined = join_slabs([s.export() for s in shards], full["global_ids"])
    assert joined.counts != n0
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 1e-5)), "sharded c4 {f}", ref_order=np.argsort(full["global_ids"]))
    for s in shards:                                        # every rank holds the same body state
        b = s.read_body_poses()
        assert np.allclose(b[1]["rotation"], ref_body[1]["rotation"], atol=1e-6)
        assert np.allclose(b[1]["translation"], ref_body[1]["translation"], atol=1e-5)


@pytest.mark.parametrize("name", ["dynamic_ball3d", "dynamic_ball2d"])
def test_dynamic_bodies_on_sharded_data(hip_libs, name):
    """Two-way coupling across slabs (rigid_impulses.wgsl:94-137, p2g.wgsl:142-155): every slab accumulates the
    fixed-point impulses of its own particles, the sums are reduced over the slabs before integrate_bodies. Against
    the single-domain run of the golden scene: the bodies to the fixed-point resolution (1e-5 per node and substep:
    a node's impulse is truncated per slab here, once in a single domain), the particles to fp32 round-off."""
    from wgsparkl_amd.sharded import native_lockstep
    make, k = _CASES[name]
    sc = make()
    dim = sc["particles"].dim
    ref = run_gpu(sc, k)
    ref_p, ref_b = ref.read_particles(), ref.read_body_poses()
    pipe = pipeline(dim)
    shards, _ = lockstep_slabs(pipe, sc, 2)
    assert min(s.num_particles() for s in shards) > 0
    native_lockstep(pipe, shards, k)
    for s in shards:
        s.sync()
    bodies = [s.read_body_poses() for s in shards]
    for key in ("rotation", "translation", "linvel", "angvel"):
        a = np.stack([b[key] for b in bodies[0]])
        assert np.array_equal(a, np.stack([b[key] for b in bodies[1]])), "every slab integrates the same bodies"
        want = np.stack([b[key] for b in ref_b])
        err = float(np.abs(a - want).max())
        report_margin(f"sharded body {key} abs err", err, 3e-4)
        assert err < 3e-4, (key, a, want)
    assert np.abs(np.stack([b["linvel"] for b in bodies[0]])[0] - np.asarray(sc["colliders"][0].linvel)[:dim]).max() > 1e-3, \
        "the dynamic body must have been pushed"
    joined = join_slabs([s.export() for s in shards], np.arange(sc["particles"].n))
    assert_joined_close(joined, ref_p, (("pos", 1e-5), ("vel", 5e-5)), "sharded two-way {f}")


@pytest.mark.parametrize("dim", [3, 2])
def test_sharded_substep_with_pack_and_interior_grid_update_inside_the_p2g_launch_is_bit_identical(hip_libs, dim, monkeypatch):
    """Inside wgs_sharded_step the waves that pack the outgoing messages and the grid update of the interior blocks ride in
    the P2G launch (GU = 3: slabs handed over word by word); the interface layers are updated after the
    exchange. WGS_DEBUG GU_OWN_LAUNCH brings the k_pack_face launch and the one grid update back: the same bits on every slab
    (3 slabs in lockstep, a floor, particles migrating, a table rebuild inside the run)."""
    from wgsparkl_amd.sharded import native_lockstep
    monkeypatch.setenv("WGS_REHASH_PERIOD", "64")
    world = 3

    def run():
        if dim == 3:
            sc = scenes.config_scene("c2", world, None, "weak", n_side=24)
            sc["particles"].pos[:, 1] -= 5.6                  # in contact with the floor: both P2G bodies run
        else:
            sc = scenes.elastic_block_2d(nx=48 * world, ny=40, with_floor=True)
            sc["particles"].pos[:, 1] -= 4.6
        ps = sc["particles"]
        rng = np.random.default_rng(8)
        ps.vel[:] = rng.normal(0.0, 2.0, ps.vel.shape).astype(np.float32)
        ps.vel[:, 0] += 8.0
        pipe = pipeline(dim)
        shards, part = lockstep_slabs(pipe, sc, world)
        native_lockstep(pipe, shards, 40)
        for sh in shards:
            sh.sync()                                          # (the near-collider lists are seen here: paired launches from now on)
        native_lockstep(pipe, shards, 40)
        for sh in shards:
            sh.sync()
        return [sh.export() for sh in shards]
    a = run()
    with debug(monkeypatch, "GU_OWN_LAUNCH"):
        b = run()
    # wgs_sharded_step with neighbours splits P2G: the two block layers at each cut first (their slabs are what the messages
    # are gathered from: they run beside the exchange on a stream of their own), every other block and the interior's grid
    # update in a second launch. WGS_DEBUG SHARD_SPLIT_LAYERS splits the lockstep slabs the same way (on their one stream): same bits.
    with debug(monkeypatch, "SHARD_SPLIT_LAYERS"):
        c = run()
    # A slab's fused G2P bins its residents for the next substep (the guests it drops leave their block's total) and
    # k_g2p_arrivals the particles that arrive (Dev::bin_next); WGS_DEBUG REBIN_LAUNCH brings launch 1 of the sort, k_rebin, back:
    # the same bits, the same storage order.
    with debug(monkeypatch, "REBIN_LAUNCH"):
        e = run()
    for other in (b, c, e):
        for x, y in zip(a, other):
            x, y = by_id(x), by_id(y)                              # (the storage order of a slab follows the arrival order of its guests)
            for f in ("ids", "pos", "vel", "def_grad", "affine"):
                assert np.array_equal(x[f], y[f]), f


@pytest.mark.parametrize("world,dim", [(2, 3), (3, 3), (4, 3), (2, 2)])
def test_native_lockstep_matches_single_domain(hip_libs, world, dim, monkeypatch):
    """wgs_sharded_step_lockstep — the C++ driver of the substep protocol that wgs_sharded_step runs per rank over
    RCCL — reproduces the single-domain run (80 substeps: crosses a table rebuild; particles migrate)."""
    from wgsparkl_amd.sharded import associated_block_x, native_lockstep
    monkeypatch.setenv("WGS_REHASH_PERIOD", "64")             # table rebuilds inside the run (developer override, same results)
    # a bar along x, a few blocks per slab (a slab between two neighbours must be at least 3 blocks wide)
    if dim == 3:
        sc = scenes.config_scene("c2", world, None, "weak", n_side=24)      # 24 * world x 24 x 24 particles
        sc["colliders"] = []
    else:
        sc = scenes.elastic_block_2d(nx=48 * world, ny=40, with_floor=False)
    ps = sc["particles"]
    rng = np.random.default_rng(8)
    ps.vel[:] = rng.normal(0.0, 3.0, ps.vel.shape).astype(np.float32)
    ps.vel[:, 0] += 8.0
    k = 80
    ref = run_gpu(sc, k).read_particles()
    pipe = pipeline(dim)
    shards, part = lockstep_slabs(pipe, sc, world)
    assert part.min_interior_width() >= 3
    n0 = [s.num_particles() for s in shards]
    native_lockstep(pipe, shards, 30)
    native_lockstep(pipe, shards, k - 30)                  # two calls: state carried across frames
    for s in shards:
        s.sync()
    outs = [s.export() for s in shards]
    joined = join_slabs(outs, np.arange(ps.n))
    assert joined.exact, joined.problem
    assert joined.counts != n0, "the test scene must make particles migrate"
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 1e-5), ("def_grad", 1e-5), ("affine", 2e-4)), "native lockstep {f}")
    for r, o in enumerate(outs):                               # a rank holds its core range + the particles that left it in
        lo, hi = part.block_range(r)                           # the last substep (handed over with the next message)
        bx = associated_block_x(o["pos"], sc["cell_width"], dim)
        assert ((bx >= lo - 1) & (bx <= hi)).all()


@pytest.mark.parametrize("with_floor", [False, True])
def test_particles_enter_an_empty_slab_and_leave_theirs_empty(hip_libs, with_floor):
    """The edge of the one-exchange protocol: a cube flies from slab 0 into slab 1, which holds NO particle at the start —
    the first arrivals find none of their blocks active on their new rank and read their nodes from the message (the old
    owner's partial sums are then the totals; with the floor also the node cdfs, evaluated on the spot) — and keeps going
    until slab 0 is empty. Both against the single-domain run."""
    from wgsparkl_amd.sharded import SlabPartition, associated_block_x, native_lockstep
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=with_floor)
    ps = sc["particles"]
    if with_floor:
        ps.pos[:, 1] -= 5.6                                   # sliding just above the floor: CPIC state travels with the particles
    ps.vel[:, 0] = 400.0                                      # a third of a cell per substep
    k = 45                                                    # 15 cells: the whole cube (8 cells wide) crosses the cut
    ref = run_gpu(sc, k).read_particles()
    bx = associated_block_x(ps.pos, sc["cell_width"], 3)
    part = SlabPartition([int(bx.min()), int(bx.max()) + 1, int(bx.max()) + 12])
    pipe = pipeline(3)
    shards, _ = lockstep_slabs(pipe, sc, 2, part=part, halo_capacity_records=256, migrant_capacity=2048)
    assert [s.num_particles() for s in shards] == [ps.n, 0]
    native_lockstep(pipe, shards, 20)
    mid = [s.num_particles() for s in shards]
    assert 0 < mid[0] < ps.n and sum(mid) == ps.n, mid         # on its way
    native_lockstep(pipe, shards, k - 20)
    for s in shards:
        s.sync()
    assert [s.num_particles() for s in shards] == [0, ps.n]
    joined = join_slabs([s.export() for s in shards], np.arange(ps.n))
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 1e-5), ("def_grad", 1e-5)),
                        f"cube into an empty slab ({'floor' if with_floor else 'free'}) {{f}}")


def test_slabs_evict_the_blocks_a_body_leaves_behind(hip_libs):
    """Round 6: slabs of a decomposition evict their long-inactive blocks like single-domain data (kernels_sort.h regroup_block; until now a slab
    rebuilt its table every 1 024 substeps and whenever a moving body had used up the ids). A 16^3 cube flies through three slabs at a third of
    a cell per substep, with a block capacity that 150 substeps of its trail would exhaust: every slab builds its table once, ids come back
    on the free lists, nothing overflows, and the particles are those of the single-domain run."""
    from wgsparkl_amd.sharded import SlabPartition, associated_block_x, native_lockstep
    sc = scenes.neo_hookean_cube(n_side=16, with_floor=False)
    ps = sc["particles"]
    ps.vel[:, 0] = 400.0
    ps.vel[:, 1] = 0.0
    sc["params"] = SimulationParams((0.0, 0.0, 0.0), sc["params"].dt)
    sc["grid_capacity"] = 256                                  # the cube holds ~64 blocks at a time and touches ~40 new ones every dozen substeps
    k = 150                                                    # 50 cells
    ref_data = run_gpu(sc, k)
    ref = ref_data.read_particles()
    assert ref_data.stats()["overflow"] == 0
    bx = associated_block_x(ps.pos, sc["cell_width"], 3)
    b0 = int(bx.min())
    part = SlabPartition([b0, b0 + 5, b0 + 10, b0 + 18])
    pipe = pipeline(3)
    shards, _ = lockstep_slabs(pipe, sc, 3, part=part, halo_capacity_records=512, migrant_capacity=4096)
    for _ in range(k // 10):
        native_lockstep(pipe, shards, 10)
        for s in shards:
            s.sync()
    st = [s.stats() for s in shards]
    assert all(x["overflow"] == 0 for x in st), st
    assert all(x["table_rebuilds"] <= 1 for x in st), [x["table_rebuilds"] for x in st]
    assert sum(x["block_ids_free"] + x["table_marks"] for x in st) > 0, "no slab evicted a block"
    assert [s.num_particles() for s in shards][0] == 0
    joined = join_slabs([s.export() for s in shards], np.arange(ps.n))
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 1e-5), ("def_grad", 1e-5)), "slabs evicting a body's trail {f}")


@pytest.mark.parametrize("name", ["mesh_floor3d", "polyline2d"])
def test_mesh_colliders_on_sharded_data(hip_libs, name):
    """Mesh colliders (rigid-particle samples) on slabs: every slab holds every sample, the node cdfs of the
    nodes two slabs share are computed by both from the same inputs. Two slabs in lockstep against the single-domain run of
    the golden scene: the same particles on the same side of the mesh, fields to fp32 round-off."""
    from wgsparkl_amd.sharded import native_lockstep
    make, k = _CASES[name]
    sc = make()
    dim = sc["particles"].dim
    ref = run_gpu(sc, k).read_particles()
    pipe = pipeline(dim)
    shards, _ = lockstep_slabs(pipe, sc, 2)
    assert min(s.num_particles() for s in shards) > 0
    native_lockstep(pipe, shards, k)
    for s in shards:
        s.sync()
    joined = join_slabs([s.export() for s in shards], np.arange(sc["particles"].n))
    assert joined.exact, joined.problem
    assert (ref.cdf_affinity != 0).sum() > 10, "the scene must feel its mesh"
    assert_joined_close(joined, ref, (("pos", 1e-5), ("vel", 5e-5), ("def_grad", 1e-5)), "sharded mesh {f}")


def test_native_sharded_step_over_rccl_one_rank(hip_libs):
    """wgs_comm_* + wgs_shard_attach + wgs_sharded_step with a real RCCL communicator. A second rank on the same GPU
    is refused by RCCL, so: (a) world = 1 without neighbours must reproduce wgs_step on single-domain data;
    (b) WGS_COMM_SELF_NEIGHBOURS: the rank is its own lower and upper neighbour, so every ncclSend / ncclRecv group
    of an interior rank is issued and matched (its physics is meaningless: the slab adds its own halo to itself) —
    the run must complete, keep its particles and report no error."""
    from wgsparkl_amd.sharded import INT_MAX, INT_MIN, NativeComm, NativeShard
    sc = scenes.neo_hookean_cube(n_side=24, with_floor=True)
    ps = sc["particles"]
    ps.vel[:, 0] = 2.0
    pipe = pipeline(3)
    k = 20
    ref = run_gpu(sc, k).read_particles()
    comm = NativeComm(pipe, None, 0, 1)
    gids = np.arange(ps.n, dtype=np.uint32)
    sh = NativeShard(pipe, sc["params"], ps, gids, sc["colliders"], sc["cell_width"], sc["grid_capacity"], INT_MIN, INT_MAX,
                     False, False, ps.n, sc["model"], comm=comm, halo_capacity_records=64, migrant_capacity=64)
    sh.step(k)
    sh.sync()
    out = by_id(sh.export())
    assert rel_rms(out["pos"], ref.pos) < 1e-6 and rel_rms(out["vel"], ref.vel) < 1e-5
    sh.close(); comm.close()
    # (b) self-neighbour proxy
    comm = NativeComm(pipe, None, 0, 1, flags=1)
    from wgsparkl_amd.sharded import associated_block_x
    bx = associated_block_x(ps.pos, sc["cell_width"], 3)
    sh = NativeShard(pipe, sc["params"], ps, gids, sc["colliders"], sc["cell_width"], sc["grid_capacity"], int(bx.min()), int(bx.max()) + 2,
                     True, True, int(ps.n * 1.5), sc["model"], comm=comm, halo_capacity_records=512, migrant_capacity=1024)
    ps.vel[:, 0] = 0.0
    sh2 = sh
    sh2.step(k)
    sh2.sync()
    assert sh2.num_particles() == ps.n
    sh2.close(); comm.close()


@pytest.mark.parametrize("dim", [3, 2])
def test_single_domain_data_and_a_lone_slab_answer_alike(hip_libs, dim):
    """`MpmData` and `NativeShard` are one `wgs_data` handle (pipeline.DataHandle): the same small scene with a kinematic ball that
    moves and spins, as single-domain data and as one slab without neighbours, answers `stats()` and `read_body_poses()` alike —
    the same keys, `com` among them — before any substep and after two. Host glue only: the particles are the other tests' matter."""
    from wgsparkl_amd.sharded import INT_MAX, INT_MIN, NativeShard
    if dim == 3:
        sc = scenes.neo_hookean_cube(n_side=8)                         # 512 particles, cells 20..24 x 8..12 x 20..24
        ball = Collider.ball(1.5, (22.0, 5.5, 22.0), linvel=(0.5, 0.25, -0.75), angvel=(0.3, -0.2, 0.4))
    else:
        sc = scenes.elastic_block_2d(nx=22, ny=22, with_floor=False)   # 484 particles, cells 7..18 x 7..18
        ball = Collider.ball(1.5, (12.0, 4.5), linvel=(0.5, 0.25, 0.0), angvel=(0.3,))
    ps, cols = sc["particles"], [ball]
    pipe, data = new_data(sc, colliders=cols)
    slab = NativeShard(pipe, sc["params"], ps, np.arange(ps.n, dtype=np.uint32), cols, sc["cell_width"], sc["grid_capacity"],
                       INT_MIN, INT_MAX, has_lower=False, has_upper=False, particle_capacity=ps.n, model=sc["model"], comm=None)

    def alike(when):
        data.sync()
        slab.sync()
        assert data.stats()["num_particles"] == slab.stats()["num_particles"] == ps.n, when
        a, b = data.read_body_poses(), slab.read_body_poses()
        assert len(a) == len(b) == 1
        assert set(a[0]) == set(b[0]) == {"rotation", "translation", "linvel", "angvel", "com"}, when
        for key in a[0]:
            assert a[0][key].shape == b[0][key].shape, (when, key)
            err = max_abs(a[0][key], b[0][key])
            print(f"dim {dim} {when}: body {key} abs difference {err:.3e} (bound {FUZZ_BODY_ATOL:g})")
            assert err <= FUZZ_BODY_ATOL, (when, key, a[0][key], b[0][key])
        return a[0]

    start = alike("before any substep")
    pipe.step(data, 2)
    slab.step(2)
    moved = alike("after two substeps")
    assert not np.array_equal(moved["translation"], start["translation"]), "the ball must have moved"


def test_a_refused_lockstep_call_leaves_the_slabs_usable(hip_libs):
    """wgs_sharded_step_lockstep lends every slab slab 0's stream for the length of the call; a call it refuses must hand every
    slab its own stream back. Two pairs of slabs of one small 2D block under a resting ball: on the first pair only slab 0 is
    given the ball's mass, so the call is refused (two-way coupling on some slabs); then slab 1 gets the same mass and the pair
    runs three lockstep substeps. The second pair had the mass on both slabs from the start and runs the same three: the two
    pairs hold the same particles and bodies, bit for bit."""
    from wgsparkl_amd._ffi import WgsError
    from wgsparkl_amd.sharded import native_lockstep
    from gpu_common import export_state_and_cdf
    sc = scenes.elastic_block_2d(nx=24, ny=16, with_floor=False)          # 384 particles, cells 7..19 x 7..15
    ball = Collider.ball(1.5, (13.0, 16.0))                               # at rest, overlapping the block's top: not moving until it has a mass
    heavy = ball.with_density(500.0, 2)
    ps = sc["particles"]
    pipe = pipeline(2)
    first, _ = lockstep_slabs(pipe, {**sc, "colliders": [ball]}, 2)
    second, _ = lockstep_slabs(pipe, {**sc, "colliders": [heavy]}, 2)
    assert min(s.num_particles() for s in first) > 0

    first[0].set_body_mass_properties([heavy])
    with pytest.raises(WgsError) as e:
        native_lockstep(pipe, first, 3)
    assert "two-way coupling must be enabled on every slab or none" in str(e.value)
    for s in first:
        s.sync()                                                          # (each on its own stream again)
    first[1].set_body_mass_properties([heavy])

    for pair in (first, second):
        native_lockstep(pipe, pair, 3)
        for s in pair:
            s.sync()
    a, b = export_state_and_cdf(first, ps.n, 2), export_state_and_cdf(second, ps.n, 2)
    for f in a[0]:
        assert np.array_equal(a[0][f].view(np.uint32), b[0][f].view(np.uint32)), f
    assert np.array_equal(a[1], b[1]), "the same slab holds each particle"
    for k, name in ((2, "cdf_affinity"), (3, "cdf_dist"), (4, "cdf_normal")):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), name
    for r in range(2):
        pa, pb = first[r].read_body_poses(), second[r].read_body_poses()
        for key in pa[0]:
            assert np.array_equal(pa[0][key], pb[0][key]), (r, key)
    assert first[0].read_body_poses()[0]["linvel"][1] != 0.0, "the ball has a mass now: gravity and the block move it"


def test_lockstep_slabs_builds_what_the_spelled_slabs_build(hip_libs):
    """sharded.lockstep_slabs is split_scene + NativeShard + set_fluid_eos per slab: a Tait fluid block with exponent 5 (with the
    default 7 a forgotten setter would pass), stirred so that it compresses, as two lockstep slabs built both ways, four substeps
    each — every field of the two export()s equal bit for bit; slabs built without the exponent (`fluid_gamma=None`) end elsewhere."""
    from wgsparkl_amd.sharded import NativeShard, SlabPartition, associated_block_x, native_lockstep, split_scene, uniform_material_of
    sc = scenes.tait_fluid_block(32, 16, 16, with_floor=False, gamma=5.0)
    ps = sc["particles"]
    ps.vel[:] = np.random.default_rng(8).normal(0.0, 3.0, ps.vel.shape).astype(np.float32)
    pipe = pipeline(3)
    part = SlabPartition.balanced(associated_block_x(ps.pos, sc["cell_width"], 3), 2)
    spelled = []
    for r, (sub, gids) in enumerate(split_scene(ps, part, sc["cell_width"])):
        lo, hi = part.block_range(r)
        spelled.append(NativeShard(pipe, sc["params"], sub, gids, sc["colliders"], sc["cell_width"], sc["grid_capacity"], lo, hi, r > 0, r < 1,
                                   particle_capacity=ps.n, model=sc["model"], uniform_material=uniform_material_of(ps)))
    for s in spelled:
        s.set_fluid_eos(sc["fluid_gamma"])
    built, built_part = lockstep_slabs(pipe, sc, 2)
    assert built_part == part and min(s.num_particles() for s in built) > 0
    forgotten, _ = lockstep_slabs(pipe, sc, 2, fluid_gamma=None)
    for shards in (spelled, built, forgotten):
        native_lockstep(pipe, shards, 4)
        for s in shards:
            s.sync()

    for r, (a, b) in enumerate(zip(spelled, built)):     # (the slots of a slab are not in a reproducible order: its particles are named by their global ids)
        ea, eb = by_id(a.export()), by_id(b.export())
        assert set(ea) == set(eb) and len(ea["ids"]) > 0
        for f in ea:
            assert ea[f].tobytes() == eb[f].tobytes(), (r, f)
    assert any(by_id(a.export())["vel"].tobytes() != by_id(c.export())["vel"].tobytes() for a, c in zip(spelled, forgotten)), "the exponent does not matter here"
