"""-m gpu: the plastic particle update IN MOTION, per particle against the fp64 truth of tests/plastic_truth.py (validated on
the CPU by tests/test_plastic_truth.py): F_trial = F + (grad dt) F, the fracture test, the Drucker-Prager projection and the
stress inside one invocation of the fused G2P (g2p_body.inc), and of the arrivals' kernel (arrivals_body.inc) in a lockstep
slab decomposition.

Every checked substep of single-domain data is judged twice:
- isolated: the same state stripped of plasticity (plastic_truth.strip) is run beside it. P2G does not read the plastic state, so
  the twin's x and v are the plastic run's bit for bit and its def_grad is the kernel's own fp32 F_trial. Every particle the plastic
  run did not project holds exactly that matrix; every projected one is judged by devmath_truth's bands of that exact matrix
  (f_err = 0), the ones test_gpu_constitutive measures at rest;
- end to end: against the truth of the fp64 F_trial with f_err = b_F (wider bands, wider tolerances: plastic_truth's docstring).
Blocks, cells and the grid as in test_gpu_transfer; x, v and C' of every particle and F of the unprojected ones through
transfer_truth.check_particles; what a substep must not touch is compared bit for bit."""
import contextlib

import numpy as np
import pytest

import plastic_truth as PT
import transfer_truth as T
from gpu_common import _start, _step, check_blocks, checked_plastic_substep, plastic_twin, steady_plastic_substep
from helpers import compare_grids, debug, grid_of, pipeline, report_margin, run_oracle

pytestmark = pytest.mark.gpu

CASE_IDS = [(case, d) for case in sorted(PT.CASES) for d in (2, 3)]


def _count(name, found, at_least=0):
    """a count the test is built for, in the margins file as (required, found): value <= bound says the condition is met"""
    report_margin(f"{name} (required / found)", at_least, int(found))


def _check(tag, sc, before, got, twin, grid, poses, fam, fails, extra_levels=0.0, min_branch=0):
    """the checks of one substep from the state `before` (a ParticleSet with its dp_state and phase): gpu_common's of every plastic
    substep, then the two Drucker-Prager verdicts, which are returned."""
    d, n, model = before.dim, before.n, sc["model"]
    pt, iso, keep = checked_plastic_substep(tag, sc, before, got, twin, grid, poses, model, fails, extra_levels)
    T.check_particles(f"{tag} twin end to end", pt, twin, model, fails, sel=keep)      # within b_F of the truth both ways
    # ---- isolated: the truth of that exact fp32 matrix
    pl_iso = PT.Plastic(T.mat(twin.def_grad, d), None, before.dp, before.dp_state, before.phase)
    jd_iso = PT.judge(f"{tag} isolated", pl_iso, got, fails, F_trial32=twin.def_grad, fam=fam)
    PT.report_ambiguous(f"{tag} isolated", jd_iso, PT.AMBIGUOUS_MAX, fails)
    T.check_particles(f"{tag} isolated G2P", iso, got, model, fails, sel=keep, own_F=jd_iso.changed)
    same = ~jd_iso.changed & (got.phase[:, 0] == before.phase[:, 0])
    assert np.array_equal(got.def_grad[same], twin.def_grad[same]) and np.array_equal(got.dp_state[same], before.dp_state[same])
    _count(f"{tag}: unprojected and unbroken particles holding the twin's F bit for bit", same.sum(), int(np.ceil(0.1 * n)))
    assert same.sum() >= 0.1 * n, f"{tag}: only {int(same.sum())} of {n} particles are left unprojected and unbroken"
    # ---- end to end
    pl = PT.Plastic(pt.F, pt.b_F, before.dp, before.dp_state, before.phase)
    jd = PT.judge(f"{tag} end to end", pl, got, fails, fam=fam)
    PT.report_ambiguous(f"{tag} end to end", jd, PT.NEAR_MAX, fails)
    T.check_particles(f"{tag} end to end", pt, got, model, fails, sel=keep, own_F=jd.changed)
    for br in "ABN":
        _count(f"{tag}: particles on branch {br} (isolated verdict)", (jd_iso.branch == br).sum(), min_branch)
    _count(f"{tag}: particles broken in the checked substep", ((got.phase[:, 0] == 0) & (before.phase[:, 0] != 0)).sum())
    return jd_iso, jd


@pytest.mark.parametrize("case,d", CASE_IDS)
def test_one_substep_of_moving_plastic_particles_per_particle(hip_libs, monkeypatch, case, d):
    dbg = PT.CASES[case][4]
    monkeypatch.delenv("WGS_DEBUG", raising=False)
    with debug(monkeypatch, dbg) if dbg is not None else contextlib.nullcontext():
        sc, fam = PT.scene(case, d)
        ps = sc["particles"]
        tag = f"{case} {d}D"
        pipe, data = _start(sc)
        poses = data.read_body_poses()
        got = _step(pipe, data)
        st32 = run_oracle(sc, 1, np.float32)
        check_blocks(data, st32)
        grid = data.read_grid()
        compare_grids(grid[:2], grid_of(st32))
        twin = plastic_twin(sc)
    fails = []
    jd_iso, _ = _check(tag, sc, ps, got, twin, grid, poses, fam, fails, min_branch=10 if PT.CASES[case][2] else 0)
    assert not fails, "\n".join(fails)
    if PT.CASES[case][2]:
        assert min(int((jd_iso.branch == br).sum()) for br in "ABN") >= 10


@pytest.mark.parametrize("case,d,h", PT.STEADY)
def test_steady_state_substep_of_moving_plastic_particles(hip_libs, case, d, h):
    """k - 1 = 15 substeps, read back (plastic state and phase included), the 16th checked against the truth of the read-back
    state; the twin is new data made of that state without plasticity (a restart continues bit for bit:
    test_checkpoint_restart_is_bit_exact). Clean and dirty blocks, cell changers, k_regroup's arrivals and particles that were
    projected before are what this substep runs on."""
    sc, fam = PT.scene(case, d, h=h, steady=True)
    tag = f"steady state {case} {d}D"
    before, got, twin, grid, s0, s1 = steady_plastic_substep(sc, 15)
    _count(f"{tag}: cell changers in the checked substep", s1["cell_changers"] - s0["cell_changers"], 1)
    fails = []
    jd_iso, jd = _check(tag, sc, before, got, twin, grid, None, fam, fails)
    assert not fails, "\n".join(fails)
    again = jd_iso.changed & np.any(before.dp_state != np.array([1.0, 1.0, 0.0], np.float32), axis=1)
    moved = np.any(T.assoc_cell(before.pos, h) != T.assoc_cell(got.pos, h), axis=1)
    _count(f"{tag}: projected in the checked substep and before it", again.sum(), 20)
    _count(f"{tag}: changed cell and projected in the checked substep", (moved & jd_iso.changed).sum(), 20)
    assert again.sum() >= 20 and (moved & jd_iso.changed).sum() >= 20, (int(again.sum()), int((moved & jd_iso.changed).sum()))


# ------------------------------------------------------------------------------------------------ the arrivals' kernel
def drifting_plastic(d, h, world):
    """test_gpu_transfer's drifting clusters, plastic and breakable (plastic_truth.scene with their positions and velocities:
    deformations near I, a softer material, max_stretch in the window around s_max(F_in); all but the leading plastic_truth.SLAB_LEAD cells of the clusters that cross a
    cut are elastic)"""
    from test_gpu_transfer import _drifting
    base = _drifting(d, h, world, seed=30 + world + d)["particles"]
    bw = T.bw_of(d)
    x = base.pos[:, 0].astype(np.float64) / h
    cluster = np.floor(x / (10 * bw)).astype(int)
    lead = (cluster >= 1) & (x - 10 * bw * cluster < 1.0 + PT.SLAB_LEAD)
    sc, _ = PT.scene("mode1_fracture_corotated", d, h=h, steady=True, pos=base.pos, vel=base.vel.astype(np.float64), elastic=~lead)
    return sc


def _export(shards, n):
    from wgsparkl_amd.sharded import join_slabs
    joined = join_slabs([s.export(plastic=True) for s in shards], np.arange(n))
    assert joined.exact, joined.problem
    return joined.fields, joined.holder


@pytest.mark.parametrize("world,d,h", [(2, 3, 0.5), (3, 2, 0.3)])
def test_lockstep_slabs_plastic_particles_per_particle(hip_libs, world, d, h):
    """Export before and after each of six substeps of a lockstep decomposition, the plastic quads included (slabs use the
    general layout, uni_dp 0); every particle end to end against the truth of the whole domain at extra_levels = 8, as
    test_gpu_transfer's elastic slab test. All particles, the arrivals (whose update the arrivals' kernel runs), the arrivals
    into blocks inactive on the new rank and the particles within two cells of a cut are reported on their own.

    What this holds for an arrival is its branch, F' and dp_state within the end-to-end tolerances, and that the plastic quads it
    carries are its own. It does not hold its fracture decision: at this drift b_F / |F| is 0.2 - 1.2 % and nearly every breakable
    particle breaks before it arrives, so no arrival's decision on F_trial differs from the one on F_in outside the band (both counts
    are recorded below; notes/round_29.md)."""
    from wgsparkl_amd.sharded import associated_block_x, lockstep_slabs, native_lockstep
    sc = drifting_plastic(d, h, world)
    ps = sc["particles"]
    n = ps.n
    pipe = pipeline(d)
    shards, part = lockstep_slabs(pipe, sc, world, force_plastic=True)
    bw = T.bw_of(d)
    lo_hi = np.array([part.block_range(r) for r in range(world)])
    cuts = lo_hi[1:, 0] * bw
    native_lockstep(pipe, shards, 1)
    for s in shards:
        s.sync()
    pre, holder = _export(shards, n)
    for k in ("dp",):
        assert np.array_equal(pre[k], ps.dp), "the plasticity parameters did not survive the first substep"
    fails = []
    n_arr = n_inactive = n_arr_plastic = n_arr_broken = n_arr_branch = 0
    worst = {}
    for step in range(6):
        native_lockstep(pipe, shards, 1)
        for s in shards:
            s.sync()
        post, held = _export(shards, n)
        inp = T.Inputs(pre["pos"], pre["vel"], pre["affine"], pre["def_grad"], pre["mass"], ps.init_volume, ps.lambda_, ps.mu)
        bx = associated_block_x(inp.pos32, h, d)
        arrival = (bx < lo_hi[holder, 0]) | (bx >= lo_hi[holder, 1])
        st, _, pt = T.substep(inp, h, T.DT, T.GRAVITY[:d], extra_levels=8.0)
        nblk = st.node[..., 0] // bw
        owner = part.owner_of_blocks(bx)
        inactive = np.zeros(n, bool)
        for q in range(world):
            have = set(np.unique(nblk[(owner == q) & ~arrival]).tolist())
            a = np.nonzero(arrival & (owner == q))[0]
            inactive[a] = [any(int(b) not in have for b in nblk[i]) for i in a]
        near_cut = np.min(np.abs(st.node[:, 0, 0][:, None] + 1 - cuts[None, :]), axis=1) <= 2
        tag = f"plastic slabs {world}x {d}D h={h} substep {step}"
        assert np.array_equal(post["dp"], ps.dp), f"{tag}: the plasticity parameters changed"
        pl = PT.Plastic(pt.F, pt.b_F, pre["dp"], pre["dp_state"], pre["phase"])
        jd = PT.judge(f"{tag} all", pl, post, fails)
        PT.report_ambiguous(f"{tag} all", jd, PT.NEAR_MAX, fails)
        for name, sel in (("all", None), ("arrivals", arrival), ("arrivals into blocks inactive on the new rank", inactive),
                          ("within two cells of a cut", near_cut)):
            T.check_particles(f"{tag} {name}", pt, post, sc["model"], fails, sel=sel, own_F=jd.changed)
            m = jd.cand if sel is None else jd.cand & sel
            if sel is not None and m.any():
                w = float(np.where(jd.branch[m] == "?", np.inf, jd.ratio[m]).max())
                worst[name] = max(worst.get(name, 0.0), w)
                report_margin(f"{tag} {name}: Drucker-Prager F / state, worst error / bound (branch-matched)", w, 1.0, n=int(m.sum()),
                              off=int((jd.bad & sel).sum()))
        broke = (post["phase"][:, 0] == 0) & (pre["phase"][:, 0] != 0)
        # how many arrivals this substep DECIDES: the fp64 decision on F_trial differs from the one on F_in, outside every band
        pl_in = PT.Plastic(inp.F, None, pre["dp"], pre["dp_state"], pre["phase"])
        n_arr_broken += int((arrival & (pl.broken != pl_in.broken) & ~pl.amb_frac).sum())
        n_arr_branch += int((arrival & pl.cand64 & pl_in.cand64 & (pl.label != pl_in.label) & ~jd.amb & ~jd.pure).sum())
        n_arr += int(arrival.sum())
        n_inactive += int(inactive.sum())
        n_arr_plastic += int((arrival & (jd.changed | broke)).sum())
        pre, holder = post, held
    for s in shards:
        s.close()
    _count(f"plastic slabs {world}x {d}D: arrivals in the checked substeps", n_arr, 20)
    _count(f"plastic slabs {world}x {d}D: arrivals into blocks inactive on the new rank", n_inactive, 2)
    _count(f"plastic slabs {world}x {d}D: arrivals projected or broken in the substep they arrive in", n_arr_plastic, 5)
    _count(f"plastic slabs {world}x {d}D: arrivals whose fracture decision on F_trial is not the one on F_in, outside the band", n_arr_broken)
    _count(f"plastic slabs {world}x {d}D: arrivals whose branch on F_trial is not the one on F_in, outside the bands", n_arr_branch)
    assert not fails, "\n".join(fails)
    assert n_arr >= 20 and n_inactive >= 2 and n_arr_plastic >= 5, (n_arr, n_inactive, n_arr_plastic)
