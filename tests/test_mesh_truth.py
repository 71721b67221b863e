"""CPU: the fp64 truth of the node distance field of mesh colliders (tests/mesh_truth.py) and its bounds are right.

- the truth's active cells (the blocks the samples add included), node field and particle field agree with the C fp64
  oracle run pass by pass (update_rigid_particles, sort_rigid, grid_update_cdf, p2g_cdf, g2p_cdf): bits equal outside the
  undecided sets, distances to 1e-10 relative;
- the C fp32 oracle, an honest fp32 implementation, lands inside every bound; the worst ratios are reported;
- the undecided shares of the truth alone meet cdf_truth's caps on every scene, and no block's membership depends on an
  undecided sample;
- every scene holds at least 20 decided instances of the case it is named for;
- perturbed truths (strict edges, the sign of the closest vote, validity ignored, the true point-to-primitive distance, a
  2^D stencil, the cell by floor, the own-block rule ignored, + neighbours added, the highest id on ties, the pose or the
  scale not applied, end points valid in 2D, the normal reversed) are caught on the scenes that exercise them;
- without `rigid` a NodeField and active_cells are what they were: a mesh collider leaves no trace; with the `rigid` of a
  mesh out of every particle's reach they are the same again."""
import numpy as np
import pytest

import cdf_truth as CT
import mesh_truth as MT
import transfer_truth as T
from helpers import report_margin

CASES = MT.CASES
MIN_INSTANCES = 20


def _scene(name, d, h):
    """the cdf_truth.Case of MT.SCENES[name], from the cache test_cdf_truth.py shares"""
    return CT._case(MT.SCENES[name], d, h)


@pytest.mark.parametrize("name,d,h", CASES)
def test_truth_matches_the_fp64_oracle(oracle_libs, name, d, h):
    sc, prev, truth = _scene(name, d, h)
    assert sc["particles"].n <= (3000 if d == 3 else 1500)
    CT.assert_matches_fp64_oracle(sc, prev, truth)


@pytest.mark.parametrize("name,d,h", CASES)
def test_fp32_oracle_fits_the_bounds_and_the_caps_hold(oracle_libs, name, d, h):
    CT.assert_fp32_oracle_fits_and_caps_hold(name, *_scene(name, d, h))


# what every scene must hold MIN_INSTANCES decided instances of (mesh_truth.counts)
NAMED = {
    "sheet": ("positive", "negative"),                                  # nodes on both sides
    "aligned": ("on_plane", "on_edge", "no_vote"),                      # distance 0, projections exactly on an edge (2D: on an end point), one step outside
    "solid": ("two_sign", "no_vote"),
    "heightfield": ("multi_vote",),                                     # several samples per node
    "mixed": ("exact_tie", "two_colliders"),
    "mixed_mesh_first": ("exact_tie", "two_colliders"),
    "slot15": ("bit31",),
    "degenerate": ("flat_pairs", "multi_vote"),                         # pairs of primitives without area / length, decided invalid; the sound ones vote
    "lonely": ("sample_only_blocks", "sample_only_nodes_with_votes", "ignored_samples", "node_block_missing"),
}


@pytest.mark.parametrize("name,d,h", CASES)
def test_the_scenes_reach_the_edges_they_are_named_for(name, d, h):
    truth = _scene(name, d, h).truth
    rg, nf = truth.rigid, truth.nodes
    c = MT.counts(rg, nf)
    for k in NAMED[name]:
        report_margin(f"mesh {name} {d}D h={h}: decided instances of {k}", c[k], MIN_INSTANCES)
        assert c[k] >= MIN_INSTANCES, (name, d, h, k, c)
    if name.startswith("mixed"):
        mesh_id = 0 if name == "mixed_mesh_first" else 1
        tie = nf.voter[:, 0] & nf.voter[:, 1] & (nf.dist_c[:, 0] == nf.dist_c[:, 1]) & ~nf.und_tie & ~nf.und_dist
        assert tie.sum() >= MIN_INSTANCES and (nf.closest[tie] == 0).all()
        # regions where the mesh alone is nearer, and where the cuboid is
        assert ((nf.closest == mesh_id) & ~nf.und_tie).sum() >= MIN_INSTANCES and ((nf.closest == 1 - mesh_id) & ~tie).sum() >= MIN_INSTANCES
    if name == "aligned":
        P = rg.pairs
        on = P["certain"] & P["valid"] & ~P["valid_und"] & (P["dist"] == 0.0)
        assert not P["neg"][on].any() and not P["neg_und"][on].any(), "a node on the plane is decided: positive"


MESH_VARIANTS = {
    # (3D only: the 2D rule is strict already — a projection on an end point is invalid — so 2D has no closed edge to open)
    "strict_edges": [("aligned", 3)],
    "sign_of_closest": [("solid", 2), ("solid", 3)],
    "no_validity": [("solid", 2), ("solid", 3), ("heightfield", 2), ("heightfield", 3)],
    "true_distance": [("solid", 2), ("solid", 3)],
    "stencil2": [(n, d) for n in MT.SCENES for d in (2, 3)],
    "cell_floor": [(n, d) for n in MT.SCENES for d in (2, 3)],
    "no_own_block": [("lonely", 2), ("lonely", 3)],
    "adds_neighbours": [("lonely", 2), ("lonely", 3)],
    "closest_highest": [("mixed", 2), ("mixed", 3), ("mixed_mesh_first", 2), ("mixed_mesh_first", 3)],
    "no_pose_vertices": [("sheet", 2), ("sheet", 3)],
    "ignore_scale": [("sheet", 2), ("sheet", 3)],
    "endpoints_valid_2d": [("sheet", 2)],
    "reversed_normal": [("sheet", 2), ("sheet", 3)],
}


@pytest.mark.parametrize("name,d,h", CASES)
def test_perturbations_are_caught(monkeypatch, name, d, h):
    monkeypatch.setattr(T, "report_margin", lambda *a, **k: None)     # (perturbed fields are no measured margins)
    sc, _, truth = _scene(name, d, h)
    nf = truth.nodes
    pos = sc["particles"].pos
    cols = CT.colliders_of(sc["colliders"], d)
    # control: the unperturbed truth, rebuilt and rounded to fp32 like every perturbed field below, passes the same checks
    ctl = MT.rigid_of(sc)
    assert np.array_equal(CT.active_cells(pos, h, d, rigid=ctl), nf.cells)
    same = CT.NodeField(cols, d, h, nf.cells, rigid=ctl)
    fails = []
    CT.check_nodes("control", nf, same.dist.astype(np.float32), same.aff, same.closest, fails)
    assert not fails, "\n".join(fails)
    for v, where in MESH_VARIANTS.items():
        if (name, d) not in where:
            continue
        bad_rg = MT.rigid_of(sc, variant=(v,))
        if not np.array_equal(CT.active_cells(pos, h, d, rigid=bad_rg), nf.cells):
            continue                                                   # caught: the active cells differ
        bad = CT.NodeField(cols, d, h, nf.cells, rigid=bad_rg, variant=(v,))
        fails = []
        CT.check_nodes(v, nf, bad.dist.astype(np.float32), bad.aff, bad.closest, fails)
        assert fails, f"{v} is not caught on {name} {d}D h={h}"


@pytest.mark.parametrize("d", [2, 3])
def test_without_rigid_a_mesh_collider_leaves_no_trace(d):
    h = 0.5
    sc = MT.sheet(d, h)
    pos = sc["particles"].pos
    cols = CT.colliders_of(sc["colliders"], d)
    cells = CT.active_cells(pos, h, d)
    blk = T.assoc_cell(pos, h) // T.bw_of(d)
    assert len(cells) == 64 * len(np.unique((blk[:, None, :] + np.unique(T.shifts_of(d) % 2, axis=0)[None, :, :]).reshape(-1, d), axis=0))
    nf = CT.NodeField(cols, d, h, cells)
    assert not nf.aff.any() and not nf.und_bits.any() and (nf.closest == CT.NONE).all() and (nf.dist == CT.NO_VOTER).all()


@pytest.mark.parametrize("d", [2, 3])
def test_a_mesh_out_of_reach_gives_the_truth_without_rigid(d):
    """The scene of test_gpu_cdf.py's k_cdf path: a small mesh more than four blocks from every particle. Its Rigid adds no
    block, every sample is ignored, and the node field is the one built without `rigid`, element for element."""
    h = 0.5
    sc = MT.far_mesh(CT.two_equal(d, h))
    pos = sc["particles"].pos
    rg = MT.rigid_of(sc)
    cells = CT.active_cells(pos, h, d)
    assert np.array_equal(CT.active_cells(pos, h, d, rigid=rg), cells)
    assert rg.n > 0 and len(rg.sample_only) == 0 and rg.ignored.all() and not rg.und_blocks
    cols = CT.colliders_of(sc["colliders"], d)
    bare, full = CT.NodeField(cols, d, h, cells), CT.NodeField(cols, d, h, cells, rigid=rg)
    for f in ("dist", "aff", "closest", "und_bits", "und_dist", "und_tie", "b_dist"):
        assert np.array_equal(getattr(bare, f), getattr(full, f)), f
    both = CT.truth_of(sc)
    assert both.rigid is not None and np.array_equal(both.nodes.cells, cells) and np.array_equal(both.nodes.aff, bare.aff)
