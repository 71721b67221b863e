"""-m gpu: the node distance field of mesh colliders (trimesh, heightfield, polyline) checked node by node against the fp64
truth of tests/mesh_truth.py (its bounds are settled on the CPU by tests/test_mesh_truth.py), through k_rigid_transform,
k_rigid_mark / k_rigid_touch, k_p2g_cdf, the reset of its accumulators in the sort and the merge in k_cdf.

Every checked substep (gpu_common.checked_substep): the positions, previous affinity words and collider
poses are those read before it; after it the active cells are exactly the truth's (the blocks the samples add included, and
none that depends on an undecided sample), every node's affinity / sign bits and closest id are exact outside the undecided
sets and its distance is within its bound, nodes with no voter hold exactly (1e10, NONE, 0), every particle is checked from
the kernel's own node field (isolated) and from the truth's (end to end), and the caps on the undecided shares hold."""
import contextlib
import dataclasses

import numpy as np
import pytest

import cdf_truth as CT
import mesh_truth as MT
import transfer_truth as T
from gpu_common import blocks_in_reach, check_blocks, check_lockstep_slabs, checked_substep
from helpers import debug, new_data, pipeline, report_margin, run_oracle
from wgsparkl_amd.sharded import lockstep_slabs
from wgsparkl_amd.solver import Collider

pytestmark = pytest.mark.gpu

CASES = MT.CASES


@pytest.mark.parametrize("name,d,h", CASES)
def test_mesh_shapes_one_substep(hip_libs, name, d, h):
    i = CASES.index((name, d, h))
    sc = MT.SCENES[name](d, h, uniform=i % 2 == 1)          # (the two layouts alternate)
    data = new_data(sc)[1]
    fails = []
    checked_substep(f"mesh {name} {d}D h={h}", sc, data, fails, first=True)
    check_blocks(data, run_oracle(sc, 1, np.float32))
    assert not fails, "\n".join(fails)


WIDTH = {3: 3.9, 2: 0.15}     # extent of the moving sheet (2D: of each of its two segments) along its path, in h
TRAVEL = 0.4          # h per substep


def _moving_mesh_scene(d, h, x0=None, plastic=False):
    """A fixed heightfield (3D) / polyline (2D) under a bed of particles six blocks long, and a kinematic tilted sheet well
    above the bed (its reach ends above the highest node that receives mass, so it takes no impulse and its velocity is
    not limited) that travels along x at 0.4 h per substep while it turns slowly.

    3D: the sheet rises along z and starts in the z blocks before the bed's: there its samples' own blocks hold no particle
    and are no + neighbour of one that does, while their + neighbours in z are: blocks that exist only because a sample
    adds them, one per block along x, which appear as the sheet's front enters a block and disappear as its back leaves
    one. The sheet is 3.9 h long, a block less 0.1 h: its front crosses into a block 0.25 h from the start and 4 h on, its
    back 0.1 h before each (no edge of it ever lies in a node plane).
    2D: the bed has a gap two blocks long: the first is the + neighbour of the bed's, the second exists only where a
    sample adds it. The sheet is two steep segments over two rows of blocks, a block and a half apart: the front one leaves
    the second block of the gap (its two blocks disappear), later the rear one enters it (they appear again).
    x0: where the sheet's reference point starts (in h); default: as described."""
    bw, W = T.bw_of(d), WIDTH[d]
    rng = np.random.default_rng(60 + d)
    top = 2 * bw + 3.0                                    # of the bed
    y_sheet = 2 * bw + 6.2                                # (mass reaches nodes up to top + 1.5 h; the sheet's votes start 1.5 h below it)
    vel = (float(np.float32(TRAVEL * h / T.DT)), 0.0, 0.0)
    if d == 3:
        ii, jj = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
        hts = (0.5 * np.sin(0.9 * ii) * np.cos(0.7 * jj)).astype(np.float32)
        fixed = Collider.heightfield(hts, tuple(float(np.float32(v * h)) for v in (6.4 * bw, 0.6, 3.0 * bw)),
                                     CT._v(np.array([3.0 * bw + 0.13, bw - 0.3, 1.5 * bw + 0.21]) * h, d), rotation=CT.ident(d))
        L = 2.2 * bw
        v = np.array([[0, 0, 0], [W, 0, 0], [0, 0, L], [W, 0, L]], np.float32) * np.float32(h)
        if x0 is None:
            x0 = 3 * bw + 0.5 - 0.25 - W                  # (a sample at x lies in cell rint(x / h) - 1: the front is 0.25 h short of block 3)
        sheet = Collider.trimesh(v, np.array([[0, 1, 2], [2, 1, 3]], np.uint32), CT._v(np.array([x0, y_sheet, 0.3 * bw]) * h, d),
                                 rotation=CT._quat((1.0, 0.0, 0.0), -10.0), linvel=vel, angvel=(float(np.float32(-0.01 / T.DT)), 0.0, 0.0))
        boxes = [(np.array([1.0, bw + 0.5, bw + 1.2]) * h, np.array([6 * bw - 1.0, top, 2 * bw + 2.5]) * h)]
    else:
        x = np.linspace(-0.2 * bw, 6.2 * bw, 9)
        v = np.stack([x, 0.3 * np.sin(0.9 * np.arange(9))], 1).astype(np.float32) * np.float32(h)
        fixed = Collider.polyline(v, np.stack([np.arange(8), np.arange(1, 9)], 1).astype(np.uint32),
                                  CT._v(np.array([0.13, bw - 0.3]) * h, d), rotation=CT.ident(d))
        gap = bw + 4.0                                    # between the two segments
        v = np.array([[0, 0], [W, 3.3], [gap, 0], [gap + W, 3.3]], np.float32) * np.float32(h)
        if x0 is None:
            x0 = 4 * bw + 0.5 - 0.35 - gap                # (the back of the front segment leaves block 3 after 0.35 h)
        sheet = Collider.polyline(v, np.array([[0, 1], [2, 3]], np.uint32), CT._v(np.array([x0, y_sheet]) * h, d), rotation=CT.ident(d),
                                  linvel=vel, angvel=(float(np.float32(0.002 / T.DT)),))
        boxes = [(np.array([1.0, bw + 0.5]) * h, np.array([2 * bw - 1.2, top]) * h),
                 (np.array([4 * bw + 1.6, bw + 0.5]) * h, np.array([6 * bw - 1.0, top]) * h)]
    sc = MT._static(d, h, rng, [fixed, sheet], boxes, 3000 if d == 3 else 1500, rim_keep=1.0)
    if plastic:
        from wgsparkl_amd.models import DruckerPrager, ElasticCoefficients
        from wgsparkl_amd.solver import ParticleSet
        sc["particles"] = ParticleSet.uniform(sc["particles"].pos, h / 4.0, 10.0, ElasticCoefficients.from_young_modulus(1e5, 0.3),
                                              plasticity=DruckerPrager.new(1e5, 0.25), phase=None)
    return sc, fixed, sheet


def _at_pose(c, pose, d):
    """the collider at a pose read back from the library"""
    rot = tuple(float(v) for v in pose["rotation"]) if d == 3 else (float(np.arctan2(pose["rotation"][1], pose["rotation"][0])),)
    return dataclasses.replace(c, translation=tuple(float(v) for v in pose["translation"]), rotation=rot)


PATHS = [("default", 2), ("default", 3), ("NO_REBIN", 2), ("NO_REBIN", 3), ("REBIN_LAUNCH", 3), ("plastic", 3)]


@pytest.mark.parametrize("path,d", PATHS)
def test_node_field_follows_a_moving_mesh(hip_libs, monkeypatch, path, d):
    """12 substeps of the moving-mesh scene, each checked with the poses read before it: the accumulators k_p2g_cdf scatters
    into are those of this substep in every block it can write to — blocks the steady-state sort leaves alone, blocks that
    hold no particle and exist only because a sample touched them —, such a block survives the sort's eviction while
    samples keep it and leaves when the mesh moves on. Paths: the default; NO_REBIN (the particles are never re-binned
    in between); REBIN_LAUNCH (the sort's first launch back); Drucker-Prager data, whose fused G2P does not bin. Then the
    fixed mesh moves by 0.37 h (set_colliders): everything kept from before is stale."""
    h = 0.2
    sc, fixed, sheet = _moving_mesh_scene(d, h, plastic=path == "plastic")
    with debug(monkeypatch, path) if path in ("NO_REBIN", "REBIN_LAUNCH") else contextlib.nullcontext():
        data = new_data(sc)[1]
    fails = []
    entered, left, appeared, gone, reach, only = set(), set(), set(), set(), None, None
    for k in range(12):
        chk = checked_substep(f"moving mesh {path} {d}D substep {k}", sc, data, fails, first=k == 0)
        now, lone = blocks_in_reach(chk.nodes, 1, d), set(map(tuple, chk.rigid.sample_only.tolist()))
        if reach is not None:
            entered |= now - reach
            left |= reach - now
            appeared |= lone - only
            gone |= only - lone
        reach, only = now, lone
    for what, s in (("entered the sheet's reach", entered), ("left the sheet's reach", left), ("exist only for a sample: appeared", appeared),
                    ("exist only for a sample: disappeared", gone)):
        report_margin(f"moving mesh {path} {d}D: blocks that {what}", len(s), 2)
    poses = data.read_body_poses()
    moved = [dataclasses.replace(_at_pose(fixed, poses[0], d), translation=CT._v(np.asarray(fixed.translation) + np.array([0.0, 0.37 * h, 0.0])[:d], d)),
             _at_pose(sheet, poses[1], d)]
    data.set_colliders(moved)
    checked_substep(f"moving mesh {path} {d}D after the fixed mesh moved", sc, data, fails, first=False, colliders=moved)
    assert not fails, "\n".join(fails)
    assert min(len(entered), len(left), len(appeared), len(gone)) >= 2, (len(entered), len(left), len(appeared), len(gone))


@pytest.mark.parametrize("d", [2, 3])
def test_lockstep_slabs_with_a_mesh_across_the_cut(hip_libs, d):
    """The moving-mesh scene as two lockstep slabs, 4 substeps: the sheet's reach starts short of the cut and crosses it.
    Every particle against the truth of the whole domain; the nodes of each slab's own blocks against the truth restricted
    to them; no collider-affine node of a slab's range is missing."""
    h = 0.2
    bw = T.bw_of(d)
    sc, _, _ = _moving_mesh_scene(d, h)
    ps = sc["particles"]
    pipe = pipeline(d)
    shards, part = lockstep_slabs(pipe, sc, 2)
    cut = part.block_range(1)[0]
    for s in shards:
        s.close()
    # 2D: the steep front segment votes up to the node 1.5 h ahead of it: one node short of the cut at the start. 3D: a node
    # ahead of the sheet's front edge does not project on it: the edge itself starts 0.85 h short of the cut's node plane.
    # (Neither puts a sample at half a cell or an edge in a node plane in any of the 4 substeps.)
    front = cut * bw - (2.45 if d == 2 else 0.85)
    x0 = front - WIDTH[d] if d == 3 else front - WIDTH[d] - (bw + 4.0)
    sc, fixed, sheet = _moving_mesh_scene(d, h, x0=x0)
    assert np.array_equal(sc["particles"].pos, ps.pos)
    shards, part = lockstep_slabs(pipe, sc, 2)
    fails = []
    crossed = check_lockstep_slabs(f"slabs moving mesh {d}D", sc, shards, part, 4, fails)
    for s in shards:
        s.close()
    report_margin(f"slabs moving mesh {d}D: substeps in which the sheet's reach is past the cut", sum(crossed), 1)
    assert not fails, "\n".join(fails)
    assert not crossed[0] and crossed[-1], crossed
