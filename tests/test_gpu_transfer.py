"""-m gpu: P2G, the grid update, G2P and the particle update checked node by node and particle by particle against the fp64
truth of tests/transfer_truth.py (its bounds are validated on the CPU by tests/test_transfer_truth.py).

Every checked substep: blocks and cells exactly (check_blocks, the active node set), every node's mass and velocity, every
particle's x, v, F and C' twice — from the kernel's own read-back grid (isolated G2P truth) and end to end. C' takes the
stress in fp64 from the kernel's own F' (test_gpu_devmath checks the stress itself). Scenes: every subset of a block's 2^D
source blocks, cell occupancies around the rounds of four ranks, coordinates across 0 and at the edges of the packed key
range, h in {0.2, 0.3, 0.5, 2}, exact ties and one-ulp neighbours of them, velocities straddling h / dt, gravity with
every component non-zero; steady-state substeps (clean blocks, dirty blocks, arrivals of k_regroup); a lockstep slab
decomposition whose checked substep carries arrivals."""
import numpy as np
import pytest

import transfer_truth as T
from gpu_common import check_blocks
from helpers import compare_grids, grid_of, pipeline, report_margin, run_gpu, run_oracle
from wgsparkl_amd.sharded import join_slabs, lockstep_slabs

pytestmark = pytest.mark.gpu

NEAR_MAX = 0.05      # fraction of nodes / particles whose truth lies within its bound of h / dt (either side accepted)
CASES = [(name, d, h) for name in T.SCENES for d in (2, 3) for h in (0.2, 0.3, 0.5, 2.0)]


def _check_substep(tag, inp, h, model, cells, vm, got, fails, extra_levels=0.0):
    d = inp.d
    st, gr, pt = T.substep(inp, h, T.DT, T.GRAVITY[:d], extra_levels=extra_levels)
    near_n, nn = T.check_grid(f"{tag} grid", gr, cells, vm, fails, extra_levels=extra_levels)
    iso = T.isolated(inp, st, cells, vm[:, :d], T.DT)
    T.check_particles(f"{tag} isolated G2P", iso, got, model, fails)
    near_p = T.check_particles(f"{tag} end to end", pt, got, model, fails)
    report_margin(f"{tag}: nodes near the clamp (fraction)", near_n / max(nn, 1), NEAR_MAX, count=near_n)
    report_margin(f"{tag}: particles near the speed cap (fraction)", near_p / inp.n, NEAR_MAX, count=near_p)
    assert near_n <= NEAR_MAX * nn and near_p <= NEAR_MAX * inp.n


@pytest.mark.parametrize("name,d,h", CASES)
def test_one_substep_node_by_node_and_particle_by_particle(hip_libs, name, d, h):
    i = CASES.index((name, d, h))
    model = i % 2
    uniform = i % 4 == 3                 # the uniform-material layout (3D: mass and material are kernel arguments)
    sc = T.SCENES[name](d, h, model=model, uniform=uniform)
    ps = sc["particles"]
    inp = T.Inputs.of(ps)
    data = run_gpu(sc, 1)
    st32 = run_oracle(sc, 1, np.float32)
    check_blocks(data, st32)
    cells, vm = data.read_grid()[:2]
    compare_grids((cells, vm), grid_of(st32))
    fails = []
    _check_substep(f"{name} {d}D h={h}", inp, h, model, cells, vm, data.read_particles(), fails)
    assert not fails, "\n".join(fails)


def _moving(d, h, stirred, seed):
    """a block of particles 3 blocks wide; stirred: a swirl of ~40 h/s plus noise (particles change cells and blocks
    within a few substeps), else at rest (clean blocks: their runs are read directly)"""
    rng = np.random.default_rng(seed)
    bw = T.bw_of(d)
    n = 3000 if d == 3 else 1500
    pos = rng.uniform(2 * bw * h, 5 * bw * h, (n, d))
    vel = np.zeros((n, d))
    if stirred:
        c = pos.mean(0)
        vel[:, 0] = -(pos[:, 1] - c[1])
        vel[:, 1] = pos[:, 0] - c[0]
        vel = vel * (40.0 / (1.5 * bw)) + rng.normal(0.0, 10.0 * h, (n, d))
    sc = T._finish(pos, h, rng, vel=vel, vel_scale=0.0 if not stirred else 1.0)
    if not stirred:
        sc["particles"].affine[:] = 0.0
    return sc


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("stirred", [True, False])
def test_steady_state_substep(hip_libs, d, stirred):
    """k - 1 substeps, read back, one more substep checked against the truth of the read-back state: clean blocks, direct
    runs, dirty blocks, k_regroup's arrivals and the binning inside the fused G2P are what this substep runs on."""
    h = 0.3 if stirred else 0.5
    sc = _moving(d, h, stirred, seed=20 + d)
    k = 16
    data = run_gpu(sc, k - 1)
    before = data.read_particles()
    s0 = data.stats()
    pipeline(d).step(data, 1)
    data.sync()
    s1 = data.stats()
    report_margin(f"steady state {d}D stirred={stirred}: cell changers in the checked substep", s1["cell_changers"] - s0["cell_changers"], 0)
    assert s1["table_rebuilds"] == s0["table_rebuilds"], "the checked substep rebuilt the table: not a steady-state substep"
    if stirred:
        assert s1["cell_changers"] > s0["cell_changers"], "no particle changed cell in the checked substep"
    cells, vm = data.read_grid()[:2]
    fails = []
    _check_substep(f"steady state {d}D stirred={stirred}", T.Inputs.of(before), h, sc["model"], cells, vm, data.read_particles(), fails)
    assert not fails, "\n".join(fails)


def _drifting(d, h, world, seed):
    """`world` clusters 5 blocks long, 10 blocks apart along x (the balanced cuts fall on the first block of clusters 1..,
    their leading particles half a cell from the cut):
    cluster 0 drifts slowly, the others move towards -x at ~0.6 h per substep, so that their leading particles cross a
    cut every substep into blocks where the new rank has no particle of its own"""
    rng = np.random.default_rng(seed)
    bw = T.bw_of(d)
    m = 600 if d == 3 else 300
    pos, vel = [], []
    for r in range(world):
        lo = np.array([(10 * r * bw + 1) * h, 2 * bw * h, 2 * bw * h][:d])      # (associated cells from block 10 r on)
        hi = np.array([(10 * r + 5) * bw * h, 4 * bw * h, 4 * bw * h][:d])
        pos.append(rng.uniform(lo, hi, (m, d)))
        v = rng.normal(0.0, 60.0 * h, (m, d))
        v[:, 0] += -600.0 * h if r else 100.0 * h
        vel.append(v)
    return T._finish(np.concatenate(pos), h, rng, vel=np.concatenate(vel))


def _export(shards, n):
    joined = join_slabs([s.export() for s in shards], np.arange(n), fields=("pos", "vel", "def_grad", "affine", "mass"))
    assert joined.exact, joined.problem
    return joined.fields, joined.holder


@pytest.mark.parametrize("world,d,h", [(2, 3, 0.5), (3, 3, 0.3), (2, 2, 0.3), (3, 2, 2.0)])
def test_lockstep_slabs_particle_by_particle(hip_libs, world, d, h):
    """Export before and after each of six substeps of a lockstep decomposition; every particle end to end against the
    truth of the whole domain. The arrivals of a checked substep (particles a rank held outside its core range before
    it), those among them whose stencil reaches a block where the new rank has no resident (the node then comes from the
    old owner's partial sum in the message), and the particles within two cells of a cut are reported on their own."""
    from wgsparkl_amd.sharded import associated_block_x, native_lockstep
    sc = _drifting(d, h, world, seed=30 + world + d)
    ps = sc["particles"]
    pipe = pipeline(d)
    shards, part = lockstep_slabs(pipe, sc, world)
    bw = T.bw_of(d)
    lo_hi = np.array([part.block_range(r) for r in range(world)])
    cuts = lo_hi[1:, 0] * bw
    native_lockstep(pipe, shards, 1)                   # (the first arrivals come in the second substep)
    for s in shards:
        s.sync()
    pre, holder = _export(shards, ps.n)
    fails = []
    n_arr = n_inactive = 0
    for step in range(6):
        native_lockstep(pipe, shards, 1)
        for s in shards:
            s.sync()
        post, held = _export(shards, ps.n)
        inp = T.Inputs(pre["pos"], pre["vel"], pre["affine"], pre["def_grad"], pre["mass"], ps.init_volume, ps.lambda_, ps.mu)
        bx = associated_block_x(inp.pos32, h, d)
        arrival = (bx < lo_hi[holder, 0]) | (bx >= lo_hi[holder, 1])
        st, _, pt = T.substep(inp, h, T.DT, T.GRAVITY[:d], extra_levels=8.0)
        nblk = st.node[..., 0] // bw                                    # [n, S] x block of every stencil node
        owner = part.owner_of_blocks(bx)
        inactive = np.zeros(ps.n, bool)
        for q in range(world):
            have = set(np.unique(nblk[(owner == q) & ~arrival]).tolist())
            a = np.nonzero(arrival & (owner == q))[0]
            inactive[a] = [any(int(b) not in have for b in nblk[i]) for i in a]
        near_cut = np.min(np.abs(st.node[:, 0, 0][:, None] + 1 - cuts[None, :]), axis=1) <= 2
        n_arr += int(arrival.sum())
        n_inactive += int(inactive.sum())
        tag = f"slabs {world}x {d}D h={h} substep {step}"
        T.check_particles(f"{tag} all", pt, post, sc["model"], fails)
        T.check_particles(f"{tag} arrivals", pt, post, sc["model"], fails, sel=arrival)
        T.check_particles(f"{tag} arrivals into blocks inactive on the new rank", pt, post, sc["model"], fails, sel=inactive)
        T.check_particles(f"{tag} within two cells of a cut", pt, post, sc["model"], fails, sel=near_cut)
        pre, holder = post, held
    for s in shards:
        s.close()
    report_margin(f"slabs {world}x {d}D: arrivals in the checked substeps", n_arr, 0)
    report_margin(f"slabs {world}x {d}D: arrivals into blocks inactive on the new rank", n_inactive, 0)
    assert not fails, "\n".join(fails)
    assert n_arr >= 20 and n_inactive >= 2, (n_arr, n_inactive)
