"""-m gpu: the collider distance fields checked node by node and particle by particle against the fp64 truth of
tests/cdf_truth.py (closed-form signed distances; its bounds are settled on the CPU by tests/test_cdf_truth.py).

Every checked substep: the particles' positions and previous affinity words and the collider poses are those read before
it (bodies integrate at the end of a substep); after it the active cells are exactly those of the positions, every node's
affinity / sign bits and closest id are exact outside the undecided set and its distance is within its bound, nodes with
no voter hold exactly (1e10, NONE, 0); every particle's cdf_affinity is exact when decided and its cdf_dist / cdf_normal
are within their bounds, twice: from the kernel's own read-back node field (isolated) and from the truth's (end to end).
Every run asserts the caps on its undecided shares."""
import contextlib
import dataclasses

import numpy as np
import pytest

import cdf_truth as CT
import mesh_truth as MT
import transfer_truth as T
from gpu_common import blocks_in_reach, check_blocks, check_lockstep_slabs, checked_substep
from helpers import debug, new_data, pipeline, report_margin, run_oracle
from wgsparkl_amd import _ffi
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider

pytestmark = pytest.mark.gpu

CASES = [(name, d, h) for name in CT.SCENES for d in (2, 3) for h in CT.HS]


@pytest.mark.parametrize("name,d,h", CASES)
def test_shapes_and_poses_one_substep(hip_libs, name, d, h):
    i = CASES.index((name, d, h))
    sc = CT.SCENES[name](d, h, uniform=i % 2 == 1)          # (the two layouts alternate)
    if name == "sixteen":
        # the library refuses a 17th coupled collider outright (the C oracle and the truth ignore it: test_cdf_truth.py);
        # what runs here is all 16 slots in use
        with pytest.raises(_ffi.WgsError):
            new_data(sc)[1]
        sc["colliders"] = sc["colliders"][:16]
    data = new_data(sc)[1]
    fails = []
    checked_substep(f"{name} {d}D h={h}", sc, data, fails, first=True)
    check_blocks(data, run_oracle(sc, 1, np.float32))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("d", [2, 3])
def test_far_node_field_at_the_full_distance_for_h_02(hip_libs, d):
    """h = 0.2 at the full distance of the far scene: the node field alone (there the particle caps cannot hold)"""
    h = 0.2
    sc = CT.far_nodes(d, h)
    data = new_data(sc)[1]
    pipeline(d).step(data, 1)
    data.sync()
    cells, _, dist, aff, closest = data.read_grid()
    assert np.array_equal(cells, CT.active_cells(sc["particles"].pos, h, d))
    nf = CT.NodeField(CT.colliders_of(sc["colliders"], d), d, h, cells)
    fails = []
    un, cn = CT.check_nodes(f"far nodes {d}D h={h}", nf, dist, aff, closest, fails)
    report_margin(f"far nodes {d}D h={h}: undecided share of the nodes that carry an affinity", un / cn, CT.NODE_CAP, count=un, of=cn)
    assert un <= CT.NODE_CAP * cn
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("path", ["summaries", "no_summaries", "k_cdf"])
def test_each_node_field_path_agrees_with_the_truth(hip_libs, monkeypatch, path, d):
    """k_regroup with the node-cdf summaries shared between blocks (the default), without them (NO_CDF_SUMM), and k_cdf
    (a mesh collider exists; it lies out of reach and contributes no bit)"""
    h = 0.5
    sc = CT.two_equal(d, h)
    if path == "k_cdf":
        sc = MT.far_mesh(sc)
    with debug(monkeypatch, "NO_CDF_SUMM") if path == "no_summaries" else contextlib.nullcontext():
        data = new_data(sc)[1]
    fails = []
    got = checked_substep(f"node field path {path} {d}D", sc, data, fails, first=True).got
    if path == "k_cdf":
        bit = np.uint32(0x10001 << (len(sc["colliders"]) - 1))
        _, _, _, aff, _ = data.read_grid()
        assert not (aff & bit).any() and not (got.cdf_affinity & bit).any(), "the mesh collider left a bit"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("path", ["prologue_waves", "cpic_workgroups"])
def test_each_particle_field_path_agrees_with_the_truth(hip_libs, monkeypatch, path, d):
    """the particle cdf in the prologue waves of the P2G launch (the host has seen the visit list), and inside the CPIC
    workgroups (NO_PCDF_WAVES)"""
    h = 0.5
    sc = CT.capsule(d, h)
    with debug(monkeypatch, "NO_PCDF_WAVES") if path == "cpic_workgroups" else contextlib.nullcontext():
        data = new_data(sc)[1]
    pipeline(d).step(data, 1)
    data.sync()
    fails = []
    checked_substep(f"particle field path {path} {d}D", sc, data, fails, first=False)
    n_near = data.stats()["num_near_collider_blocks"]
    report_margin(f"particle field path {path} {d}D: near-collider blocks", n_near, 0)
    assert n_near > 0, "no near-collider block: the prologue-waves path was not reached"
    assert not fails, "\n".join(fails)


def _ball_scene(d, h, ball_x=None):
    """a fixed floor under a bed of particles 6 blocks long, and a kinematic ball above it moving along x at 0.4 h per substep
    (centre x = ball_x, in h; default 1.5 h into the third block)"""
    bw = T.bw_of(d)
    rng = np.random.default_rng(40 + d)
    floor = Collider.cuboid(CT._v(np.array([3.2 * bw, 1.0, 3.0 * bw]) * h, d), CT._v(np.array([3.0 * bw + 0.13, bw - 0.8, 1.5 * bw + 0.21]) * h, d),
                            rotation=CT.ident(d))
    # (the ball stays 1.6 h clear of the bed: no node inside it receives mass, so it takes no impulse, and its velocity is
    # not limited to 0.1 h / dt as that of a body in contact is)
    ball = Collider.ball(float(np.float32(1.5 * h)), CT._v(np.array([2 * bw + 1.5 if ball_x is None else ball_x, 2 * bw + 6.13, 1.5 * bw + 0.27]) * h, d),
                         linvel=(float(np.float32(0.4 * h / T.DT)), 0.0, 0.0))
    lo, hi = np.array([1.0, bw + 0.5, bw + 0.5]) * h, np.array([6 * bw - 1.0, 2 * bw + 3.0, 2 * bw + 2.5]) * h
    sc = CT._static(d, h, rng, [floor, ball], [(lo, hi)], 3000 if d == 3 else 1500, rim_keep=1.0)
    return sc, floor, ball


@pytest.mark.parametrize("d", [2, 3])
def test_kept_node_cdfs_follow_a_moving_ball_and_a_moved_floor(hip_libs, d):
    """A fixed floor under a bed of particles 6 blocks long, a kinematic ball travelling along it at 0.4 h per substep:
    the node cdfs of blocks out of the ball's reach are kept from the previous substep, those of the blocks that enter
    or leave its reach must be rebuilt. Then the floor moves by 0.37 h (set_colliders): every kept field is stale."""
    h = 0.2
    sc, floor, ball = _ball_scene(d, h)
    data = new_data(sc)[1]
    fails = []
    entered, left, reach = set(), set(), None
    for k in range(12):
        nf = checked_substep(f"moving ball {d}D substep {k}", sc, data, fails, first=k == 0).nodes
        now = blocks_in_reach(nf, 1, d)
        if reach is not None:
            entered |= now - reach
            left |= reach - now
        reach = now
    report_margin(f"moving ball {d}D: blocks that entered the ball's reach", len(entered), 2)
    report_margin(f"moving ball {d}D: blocks that left the ball's reach", len(left), 2)
    poses = data.read_body_poses()
    moved = [dataclasses.replace(floor, translation=CT._v(np.asarray(floor.translation) + np.array([0.0, 0.37 * h, 0.0])[:d], d)),
             dataclasses.replace(ball, translation=tuple(float(v) for v in poses[1]["translation"]))]
    data.set_colliders(moved)
    checked_substep(f"moving ball {d}D after the floor moved", sc, data, fails, first=False, colliders=moved)
    assert not fails, "\n".join(fails)
    assert len(entered) >= 2 and len(left) >= 2, (len(entered), len(left))


@pytest.mark.parametrize("d", [2, 3])
def test_lockstep_slabs_of_the_moving_ball_scene(hip_libs, d):
    """The moving-ball scene as two lockstep slabs, 4 substeps: the ball's reach starts 0.7 h short of the cut and crosses
    it. Every particle against the truth of the whole domain; the nodes of each slab's own blocks against the truth
    restricted to them."""
    h = 0.2
    bw = T.bw_of(d)
    sc, _, _ = _ball_scene(d, h)
    ps = sc["particles"]
    pipe = pipeline(d)
    shards, part = lockstep_slabs(pipe, sc, 2)
    cut = part.block_range(1)[0]
    for s in shards:
        s.close()
    sc, floor, ball = _ball_scene(d, h, ball_x=cut * bw - 3.7)       # (its reach ends 3 h ahead of its centre)
    assert np.array_equal(sc["particles"].pos, ps.pos)
    shards, part = lockstep_slabs(pipe, sc, 2)
    fails = []
    crossed = check_lockstep_slabs(f"slabs moving ball {d}D", sc, shards, part, 4, fails)
    for s in shards:
        s.close()
    report_margin(f"slabs moving ball {d}D: substeps in which the ball's reach is past the cut", sum(crossed), 1)
    assert not fails, "\n".join(fails)
    assert not crossed[0] and crossed[-1], crossed


@pytest.mark.parametrize("d", [2, 3])
def test_sign_persistence_under_a_thin_plate(hip_libs, d):
    """A plate of half thickness 0.3 h is swept through a layer of particles by 0.45 h per substep: a particle keeps the sign
    it had while it keeps the affinity, whatever its fresh vote says. The previous words are those read back."""
    h = 0.2
    rng = np.random.default_rng(50 + d)
    x0 = np.array([4.13, 6.21, 6.17]) * h
    at = lambda k: Collider.cuboid(CT._v(np.array([0.3, 3.0, 3.0]) * h, d), CT._v(x0 + np.array([0.45 * h * k, 0.0, 0.0]), d),
                                   rotation=CT.ident(d))
    lo, hi = np.array([3.0, 3.5, 3.5]) * h, np.array([10.0, 9.0, 9.0]) * h
    sc = CT._static(d, h, rng, [at(0)], [(lo, hi)], 3000 if d == 3 else 1500, rim_keep=1.0)
    data = new_data(sc)[1]
    fails = []
    n_kept = 0
    for k in range(8):
        # the host moves the plate (a body in contact that integrates its own velocity is limited to 0.1 h per substep)
        if k:
            data.set_colliders([at(k)])
        pf = checked_substep(f"thin plate {d}D substep {k}", sc, data, fails, first=k == 0, colliders=[at(k)]).particles
        n_kept += int(pf.fresh_sign_differs.sum())
    report_margin(f"thin plate {d}D: decided particles whose sign differs from their fresh vote", n_kept, 10)
    assert not fails, "\n".join(fails)
    assert n_kept >= 10, n_kept


def test_det_edge(hip_libs):
    """3D, h = 0.1: decided particles on both sides of det = 1e-8 carry exactly the truth's affinity word (0 below)."""
    sc = CT.det_edge()
    data = new_data(sc)[1]
    fails = []
    pf = checked_substep("det edge", sc, data, fails, first=True, part_cap=CT.DET_EDGE_CAP).particles
    dec = pf.reaches & ~pf.undecided
    below, above = int((dec & ~pf.ok).sum()), int((dec & pf.ok).sum())
    report_margin("det edge: decided particles below / above 1e-8, undecided", below, 20, above=above, undecided=int((pf.reaches & pf.undecided).sum()))
    assert below >= 20 and above >= 20
    assert not fails, "\n".join(fails)
