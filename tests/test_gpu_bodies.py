"""-m gpu: what the rigid bodies receive from the CPIC transfer and how they integrate, against the fp64 truth of
tests/body_truth.py (its bounds are validated on the CPU by tests/test_body_truth.py). gpu_common.checked_body_substep runs
one substep, checks the distance fields and the CPIC transfer (checked_cpic_substep) and then, from the kernel's own
decisions and the poses read before the substep, linvel, angvel, translation, rotation and com of every body: the impulses
go through P2G's per-wave tiles and block sums, either gather (inside the P2G launch, or the grid update's own launch), one
truncation per node, the integer atomics, and bodies_integrate_one wherever it runs (the head of the next sort launch, the
flush at the end of wgs_step, a launch of its own).

Scenes: body_truth's (ROLES: bodies below both caps, on the linear and on the angular cap, a kinematic body faster than the
caps touched and untouched, a locked axis, a rotated cuboid of unequal inertia, all 16 slots, a lone particle, node totals
of a few units), each gather path, each place the integration runs at, a steady-state substep of a stirred bed, free bodies
over 1 and 50 substeps with and without particles, and the cuboid at h = 2.0 whose accumulators leave the int32 range.

The sensitivity share (body_truth.sensitivity) is asserted >= 0.9 for every body below the caps in every checked substep
(checked_body_substep does it). The bodies below the caps are those of the `lone` scenes; see tests/test_body_truth.py for why
the dense scenes' dynamic bodies are made light enough to end on a cap instead.

The case is in the test id, not in the check names: tools/summarize_margins.py then gives the worst record per check."""
import contextlib
import dataclasses

import numpy as np
import pytest

import body_truth as BT
import cdf_truth as CT
import transfer_truth as T
from gpu_common import _bed_scene, checked_body_substep
from helpers import assert_same_bodies, debug, new_data, pipeline, report_margin, step_chunks

pytestmark = pytest.mark.gpu

CASES = BT.CASES


_NEAR = dict(near=0, bodies=0)      # over the module: a body that the last substep left ON a cap is near it in the next one


def _assert_near(tag, ck, first=True):
    """bodies near a cap (either side accepted) are counted over the module (the last test asserts at most one in ten); in a
    first substep, where no body starts on a cap, none may be"""
    _NEAR["near"] += ck.bodies.near
    _NEAR["bodies"] += len(ck.after)
    if first:
        assert ck.bodies.near <= BT.NEAR_MAX * len(ck.after), (tag, ck.bodies.near, "bodies near a cap")


@pytest.mark.parametrize("name,d,h", CASES)
def test_one_substep_body_by_body(hip_libs, name, d, h):
    i = CASES.index((name, d, h))
    sc = BT.BUILD[name](d, h, model=i % 2, uniform=i % 2 == 1)       # (the two layouts alternate)
    data = new_data(sc)[1]
    fails = []
    tag = "bodies one substep"
    ck = checked_body_substep(tag, sc, data, fails, first=True, part_cap=1.0 if name.startswith("lone") or name == "quantum" else CT.PART_CAP)
    assert not fails, "\n".join(fails)
    assert ck.impulses.in_range
    _assert_near(tag, ck)
    below = BT.reached(tag, sc, ck.impulses, ck.bodies, ck.before, ck.after)
    assert below or not name.startswith("lone")
    if name == "sixteen":
        imp = ck.impulses
        assert sorted(set(imp.body[np.abs(imp.tot).sum(1) > 0].tolist())) == list(range(16)), "not every one of the 16 bodies receives an impulse"


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("switch", [None, "GU_OWN_LAUNCH", "P2G_TWO_LAUNCHES", "NO_DIRECT_RUNS"])
def test_each_gather_path(hip_libs, monkeypatch, switch, d):
    """a node's total gathered inside the P2G launch (gu_waves), by the grid update as a launch of its own, with the two P2G
    bodies as two launches, and with every block gathered through the permutation; the first substep and the second (whose
    sort finds the particles in order: the clean blocks' direct runs that NO_DIRECT_RUNS turns off exist only from there on).
    No stat says which path a launch took: that a switch changes it rests on host_substep.inc's plan_p2g and on the
    bit-identity tests that use the same switches as references."""
    sc = BT.BUILD["two_equal"](d, 0.5)
    with debug(monkeypatch, switch) if switch else contextlib.nullcontext():
        data = new_data(sc)[1]
        fails = []
        tag = "bodies gather path"
        ck = checked_body_substep(tag, sc, data, fails, first=True)
        assert not fails, "\n".join(fails)
        assert ck.impulses.in_range
        _assert_near(tag, ck)
        BT.reached(tag, sc, ck.impulses, ck.bodies, ck.before, ck.after)
        ck = checked_body_substep(f"{tag}, second substep", sc, data, fails, first=False)
        assert not fails, "\n".join(fails)
        assert ck.impulses.in_range and ck.impulses.nodes(0) >= 1
        _assert_near(tag, ck, first=False)


@pytest.mark.parametrize("d", [2, 3])
def test_where_the_integration_runs(hip_libs, monkeypatch, d):
    """three substeps as one call (the integration rides at the head of substeps 2 and 3 and in the flush), as three calls
    (the flush every time), with the integration as a launch of its own, and without k_rebin (it rides in k_bin): the
    bodies end bit-identical, and the third substep of the three calls is checked against the truth."""
    h = 0.5
    sc = BT.BUILD["cuboid"](d, h)
    one = step_chunks(sc, (3,)).read_body_poses()
    data = step_chunks(sc, (1, 1))
    fails = []
    tag = "bodies third substep"
    ck = checked_body_substep(tag, sc, data, fails, first=False)
    assert not fails, "\n".join(fails)
    assert ck.impulses.in_range and ck.impulses.nodes(0) >= 1 and ck.bodies.bodies[0].impulse
    _assert_near(tag, ck)
    assert_same_bodies(one, ck.after)
    for switch in ("BODIES_OWN_LAUNCH", "NO_REBIN"):
        with debug(monkeypatch, switch):
            other = step_chunks(sc, (3,)).read_body_poses()
        assert_same_bodies(one, other)


def _dynamic_bed(d, h, **kw):
    """tests/test_gpu_cpic.py's bed with its ball a dynamic body light enough for the bed to put it on the linear cap (a body below the
    caps in a dense bed cannot meet the sensitivity condition, tests/test_body_truth.py)"""
    sc = _bed_scene(d, h, **kw)
    floor, ball = sc["colliders"]
    slow = dataclasses.replace(ball, linvel=tuple(float(v) for v in CT.f32(0.5 * np.asarray(ball.linvel))), angvel=tuple(float(v) for v in CT.f32(0.5 * np.asarray(ball.angvel))))
    sc["colliders"] = [floor, BT.dynamic(slow, d, h, light_mass=BT.LIGHT * 256.0)]      # (a handful of nodes push it in 2D)
    sc["roles"] = ("fixed", "linear_cap")
    return sc


@pytest.mark.parametrize("d", [2, 3])
def test_steady_state_substep(hip_libs, d):
    """8 substeps of the stirred bed with the ball sinking into it under gravity and its own velocity, then two checked ones,
    each from the state read back: the table is not rebuilt, particles change cell, the floor stays where it is."""
    h = 0.2 if d == 2 else 0.25
    sc = _dynamic_bed(d, h)
    data = new_data(sc)[1]
    start = data.read_body_poses()
    pipeline(d).step(data, 8)
    data.sync()
    fails = []
    touched = 0
    for tag in ("bodies steady state, first", "bodies steady state, second"):
        s0 = data.stats()
        ck = checked_body_substep(tag, sc, data, fails, first=False)
        s1 = data.stats()
        assert s1["table_rebuilds"] == s0["table_rebuilds"], "the checked substep rebuilt the table: not a steady-state substep"
        assert s1["cell_changers"] > s0["cell_changers"], "no particle changed cell in the checked substep"
        assert ck.impulses.in_range
        _assert_near(tag, ck, first=False)
        touched += ck.impulses.nodes(1)
        report_margin(f"{tag}: nodes that give the ball an impulse", ck.impulses.nodes(1), 0)
        assert_same_bodies(start[:1], ck.after[:1])
    assert not fails, "\n".join(fails)
    assert touched >= 1, "the ball never took an impulse in the checked substeps"


@pytest.mark.parametrize("d", [2, 3])
def test_two_lockstep_slabs(hip_libs, d):
    """the same bed as two lockstep slabs, the cut under the ball: every slab truncates the node totals of the particles it
    holds (guests included) and the group adds the integers, so the truth truncates per (node, rank); 8 substeps, then two
    checked ones. The nodes' affinities and closest ids are cdf_truth's (no pair may touch an undecided node); the poses are
    read from either rank."""
    from gpu_common import export_state_and_cdf
    from wgsparkl_amd.sharded import SlabPartition, associated_block_x, lockstep_slabs, native_lockstep
    import cpic_truth as CP
    h = 0.2 if d == 2 else 0.25
    sc = _dynamic_bed(d, h)
    ps = sc["particles"]
    pipe = pipeline(d)
    bx = associated_block_x(ps.pos, h, d)
    shards, part = lockstep_slabs(pipe, sc, 2, part=SlabPartition([int(bx.min()), 3, int(bx.max()) + 1]))     # (the ball hangs over block 3's first cell)
    bw = T.bw_of(d)
    cut = part.block_range(1)[0] * bw * h
    ball_x = shards[0].read_body_poses()[1]["translation"][0]
    assert abs(ball_x - cut) < 1.5 * h, "the cut does not run under the ball"

    def run(k):
        native_lockstep(pipe, shards, k)
        for s in shards:
            s.sync()

    run(8)
    pre, holder = export_state_and_cdf(shards, ps.n, d)[:2]
    props = BT.Props(sc["colliders"], d)
    fails = []
    both = 0
    for k, tag in enumerate(("bodies slabs, first", "bodies slabs, second")):
        before = shards[k % 2].read_body_poses()
        assert_same_bodies(before, shards[1 - k % 2].read_body_poses())
        run(1)
        post, held, aff, dist, normal = export_state_and_cdf(shards, ps.n, d)
        after = shards[1 - k % 2].read_body_poses()
        inp = T.Inputs(pre["pos"], pre["vel"], pre["affine"], pre["def_grad"], pre["mass"], ps.init_volume, ps.lambda_, ps.mu)
        nf = CT.NodeField(CT.colliders_of(sc["colliders"], d, before), d, h, CT.active_cells(inp.pos32, h, d))
        f = CP.Fields(aff, normal.astype(np.float64), dist.astype(np.float64), nf.cells, nf.aff, nf.closest)
        mo = CP.Motion.of(sc["colliders"], d, before)
        res = CP.substep(inp, h, T.DT, T.GRAVITY[:d], f, mo, extra_levels=8.0)
        p, s_ = res.grid.pairs[:2]
        und = (nf.undecided | nf.und_dist)[np.searchsorted(nf.keys, T.node_key(res.st.node[p, s_]))]
        assert not und.any(), f"{tag}: {int(und.sum())} pairs touch an undecided node"
        imp = BT.impulses(res, inp, mo, held=holder)
        ck = BT.check_bodies(f"{tag} bodies", imp, props, before, after, h, T.DT, T.GRAVITY[:d], fails)
        assert imp.in_range
        _NEAR["near"] += ck.near
        _NEAR["bodies"] += props.n
        BT.assert_sensitive(tag, ck)
        ranks = np.unique(holder[p[res.nclosest[p, s_] == 1]])
        both += len(ranks) == 2
        report_margin(f"{tag}: ranks whose particles push the ball", len(ranks), 0, nodes=imp.nodes(1))
        pre, holder = post, held
    for s in shards:
        s.close()
    assert not fails, "\n".join(fails)
    assert both >= 1, "the ball never took impulses from both slabs in one substep"


@pytest.mark.parametrize("particles", [5, 0])
@pytest.mark.parametrize("d", [2, 3])
def test_free_bodies(hip_libs, d, particles):
    """sixteen bodies that nothing touches, after 1 and after 50 substeps, on data with a few far particles (the integration
    rides in the sort launches) and on data with none (host_substep.inc leaves the integration to the next sort launch only where
    n > 0, so it runs as a launch of its own: no stat shows it, the claim rests on that line); the fixed rotated collider among
    them keeps its pose bit for bit."""
    sc = BT.free_bodies(d, particles=particles)
    data = new_data(sc)[1]
    before = data.read_body_poses()
    fails = []
    done = 0
    for count in (1, 50):
        pipeline(d).step(data, count - done)
        data.sync()
        done = count
        after = data.read_body_poses()
        BT.check_free(f"free bodies x{count}", sc, before, after, count, fails)
        assert_same_bodies(before[sc["fixed"]:sc["fixed"] + 1], after[sc["fixed"]:sc["fixed"] + 1])
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("d", [3])
def test_out_of_range(hip_libs, d):
    """the cuboid at h = 2.0: node totals saturate at +-2^31 units and the body's sums wrap modulo 2^32, like the reference; the
    body integrates what the wrapped accumulators hold. 3D only: in 2D the wrapped sums leave the body of the issue's mass below
    both caps with a sensitivity share of 0.85, short of the 0.9 every body below the caps must have, so that case is not run
    here (tests/test_body_truth.py checks the 2D accumulators themselves against the C oracle)."""
    sc = BT.out_of_range(d)
    data = new_data(sc)[1]
    fails = []
    tag = "bodies out of range"
    ck = checked_body_substep(tag, sc, data, fails, first=True)
    assert not fails, "\n".join(fails)
    imp = ck.impulses
    assert not imp.in_range and ((np.abs(imp.lo) >= (1 << 31)).any() or imp.saturating.any())
    assert ((imp.hi - imp.lo) < (1 << 29)).all(), "an interval too wide to say anything modulo 2^32"
    report_margin(f"{tag}: saturating node totals", int(imp.saturating.sum()), 0, largest_sum=float(np.abs(imp.lo).max()))


def test_at_most_one_body_in_ten_was_near_a_cap(hip_libs):
    """over every checked substep of this module that ran before this test"""
    report_margin("bodies: near a cap, over the module (share)", _NEAR["near"] / max(_NEAR["bodies"], 1), BT.NEAR_MAX, count=_NEAR["near"], bodies=_NEAR["bodies"])
    assert _NEAR["near"] <= BT.NEAR_MAX * _NEAR["bodies"], _NEAR
