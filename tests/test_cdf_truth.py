"""CPU: the fp64 truth of the collider distance fields (tests/cdf_truth.py) and its bounds are right.

- the truth's node field and particle field agree with the C fp64 oracle: bits equal outside the undecided sets, distances
  and normals to 1e-10 relative;
- where the least-squares fit is exact (one flat cuboid face) the truth equals the analytic distance and normal to 1e-12;
- the C fp32 oracle, an honest fp32 implementation, lands inside every bound; the worst ratios are reported;
- perturbed truths (another `within` test, tie rule, capsule axis, pose map, face choice, persistence, Gram matrix, output
  order) land outside them on every scene that exercises them;
- the undecided shares of the truth alone meet the caps on every scene."""
import numpy as np
import pytest

import cdf_truth as CT
import transfer_truth as T
from helpers import report_margin

CASES = [(name, d, h) for name in CT.SCENES for d in (2, 3) for h in CT.HS]


def _scene(name, d, h):
    """the cdf_truth.Case of CT.SCENES[name], from the cache test_mesh_truth.py shares"""
    return CT._case(CT.SCENES[name], d, h)


@pytest.mark.parametrize("name,d,h", CASES)
def test_truth_matches_the_fp64_oracle(oracle_libs, name, d, h):
    CT.assert_matches_fp64_oracle(*_scene(name, d, h))


@pytest.mark.parametrize("name,d,h", CASES)
def test_fp32_oracle_fits_the_bounds_and_the_caps_hold(oracle_libs, name, d, h):
    CT.assert_fp32_oracle_fits_and_caps_hold(name, *_scene(name, d, h))


@pytest.mark.parametrize("d", [2, 3])
def test_far_node_field_at_the_full_distance_for_h_02(oracle_libs, d):
    """h = 0.2 at (1000, -500, -1000) blocks: the particle caps cannot hold there (see cdf_truth.far), the node field's do"""
    h = 0.2
    sc = CT.far_nodes(d, h)
    nf = CT.NodeField(CT.colliders_of(sc["colliders"], d), d, h, CT.active_cells(sc["particles"].pos, h, d))
    un, cn = nf.share()
    report_margin(f"far nodes {d}D h={h}: undecided share of the nodes that carry an affinity", un / cn, CT.NODE_CAP, count=un, of=cn)
    assert un <= CT.NODE_CAP * cn
    prev = np.zeros(sc["particles"].n, np.uint32)
    o = CT._oracle_fields(sc, np.float64, prev)
    assert np.array_equal(o["cells"], nf.cells) and not ((o["aff"] ^ nf.aff) & ~nf.und_bits).any()
    sure = ~nf.und_dist
    assert np.all(np.abs(o["dist"][sure] - nf.dist[sure]) <= CT.REL * np.maximum(np.abs(nf.dist[sure]), h))
    o = CT._oracle_fields(sc, np.float32, prev)
    fails = []
    CT.check_nodes(f"far nodes {d}D h={h} fp32 oracle", nf, o["dist"], o["aff"], o["closest"], fails)
    assert not fails, "\n".join(fails)


def test_the_scenes_reach_the_edges_they_are_named_for():
    for d in (2, 3):
        # ball: a node exactly at a centre; the small ball still has voters
        nf = _scene("ball", d, 0.5).truth.nodes
        o = np.nonzero(np.all(nf.cells == 0, axis=1))[0]
        assert len(o) == 1 and nf.sd[o[0], 2] == -float(np.float32(0.15)) and nf.inside[o[0], 2]
        assert nf.voter[:, 1].sum() >= 4
        # cuboid: nodes and particles inside; an extent below h
        truth = _scene("cuboid", d, 0.5).truth
        nf, pf = truth.nodes, truth.particles
        assert nf.inside[:, 0].sum() >= 4 and ((pf.aff >> 16) != 0).sum() >= 20
        # aligned, power-of-two h: nodes exactly on a face are inside by equality, and decided
        nf = _scene("aligned", d, 0.5).truth.nodes
        on = nf.sd[:, 0] == 0.0
        assert on.sum() >= 8 and nf.inside[on, 0].all() and not (nf.und_bits[on] != 0).any()
        # two_equal, power-of-two h: exact decided ties, and a node in reach of three colliders
        nf = _scene("two_equal", d, 2.0).truth.nodes
        tie = nf.voter[:, 0] & nf.voter[:, 1] & (nf.dist_c[:, 0] == nf.dist_c[:, 1]) & (nf.dist_c[:, 0] == nf.dist)
        assert tie.sum() >= 1 and not nf.und_tie[tie].any() and (nf.closest[tie] == 0).all()
        assert (nf.voter[:, :3].sum(1) == 3).any()
        # sixteen: collider 16 leaves no trace although nodes are in its reach
        case = _scene("sixteen", d, 0.5)
        sc, nf = case.sc, case.truth.nodes
        assert nf.voter.shape[1] == 16 and nf.voter[:, 15].any()
        c16 = CT.colliders_of(sc["colliders"], d)[16:]
        assert CT.NodeField(c16, d, 0.5, nf.cells).voter[:, 0].any()
        # far: the block coordinates
        sc = _scene("far", d, 0.5).sc
        blk = T.assoc_cell(sc["particles"].pos, 0.5) // T.bw_of(d)
        assert np.all(np.abs(blk.mean(0) - np.array(CT.FAR_BLOCKS[d])) < 3)
        assert np.all(np.abs(np.array(CT.FAR_BLOCKS[d])) >= 1000 // (2 if d == 3 else 1))


@pytest.mark.parametrize("d", [2, 3])
def test_flat_face_anchor(d):
    """Particles whose every stencil node has affinity with the one cuboid only, lies outside it and is closest to one and
    the same flat face: the fit of a linear field is exact, so cdf_dist is the distance to the face and cdf_normal the face
    normal on the particle's side, to 1e-12. (The rotated cuboid takes its rotation in fp64 here: the matrix of an fp32
    quaternion is orthogonal to 1e-7 only, and the field of its face is linear to as much.)"""
    import math
    for name in ("rotated", "axis-aligned"):
        for h in (0.5, 2.0):
            sc = CT.cuboid(d, h, he=(3.5, 3.0, 3.3))
            cols = CT.colliders_of(sc["colliders"], d)
            c = cols[0]
            c["R"] = np.eye(d)
            if name == "rotated":
                t = math.radians(33.0)
                a = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
                c["R"] = CT.rot_matrix((math.cos(t), math.sin(t)) if d == 2 else np.append(a * math.sin(t / 2), math.cos(t / 2)), d)
            pos = sc["particles"].pos
            nf = CT.NodeField(cols, d, h, CT.active_cells(pos, h, d))
            pf = CT.from_truth_nodes(pos, h, nf)
            he = c["shape"][:d]
            x = pos.astype(np.float64)
            pl = (pf.st.node * h - c["trans"]) @ c["R"] / c["scale"]                  # [n, S, d]
            q = np.abs(pl) - he
            j = np.searchsorted(nf.keys, T.node_key(pf.st.node.reshape(-1, d)))
            only = ((nf.aff[j].reshape(len(x), -1) & 0xffff) == 1).all(1)             # every node: affinity with collider 0
            n_anchor = 0
            for k in range(d):
                other = np.delete(np.arange(d), k)
                for sgn in (1.0, -1.0):
                    # every node closest to the face (k, sgn): outside in its prism, or inside with it the least penetrated
                    face = np.all((sgn * pl[..., k] > 0.0) & np.all(q[..., other] < np.minimum(q[..., k], 0.0)[..., None], axis=-1), axis=1)
                    sel = face & only & pf.ok
                    if not sel.any():
                        continue
                    xl = (x[sel] - c["trans"]) @ c["R"] / c["scale"]
                    sd = (sgn * xl[:, k] - he[k]) * c["scale"]                     # the particle's side: cdf_dist >= 0 there
                    want_d = np.abs(sd)
                    want_n = np.sign(sd)[:, None] * sgn * c["R"][:, k][None, :]
                    err_d = float(np.max(np.abs(pf.dist[sel] - want_d)))
                    err_n = float(np.max(np.abs(pf.normal[sel] - want_n)))
                    report_margin(f"anchor {name} {d}D h={h} face {k}{'+' if sgn > 0 else '-'}: cdf_dist", err_d, 1e-12 * h, n=int(sel.sum()))
                    report_margin(f"anchor {name} {d}D h={h} face {k}{'+' if sgn > 0 else '-'}: cdf_normal", err_n, 1e-12)
                    assert err_d <= 1e-12 * h and err_n <= 1e-12, (name, d, h, k, sgn, err_d, err_n)
                    n_anchor += int(sel.sum())
            assert n_anchor >= 10, (name, d, h, n_anchor)


def test_curvature_term_of_round_shapes_is_reported():
    """The least-squares distance of a ball / capsule differs from the analytic one by a curvature term of order h^2 / r:
    reported, nothing asserted."""
    for name in ("ball", "capsule"):
        for d in (2, 3):
            h = 0.5
            sc = _scene(name, d, h).sc
            pf = CT.truth_of(sc).particles
            c = CT.colliders_of(sc["colliders"], d)[0]
            x = sc["particles"].pos.astype(np.float64)
            xl = (x - c["trans"]) @ c["R"] / c["scale"]
            _, sd, _ = CT._project(c, xl, d, ())
            sel = pf.ok & (pf.aff == 1)
            dev = np.abs(pf.dist[sel] - sd[sel] * c["scale"])
            r = (c["shape"][0] if name == "ball" else c["shape"][1]) * c["scale"]
            report_margin(f"curvature {name} {d}D h={h}: max |truth cdf_dist - analytic| (bound column: h^2 / r)", float(dev.max()), h * h / r, n=int(sel.sum()))


NODE_VARIANTS = {
    "euclid_within": list(CT.SCENES),        # (aligned: only 3D with faces on node planes has corner nodes between the two tests)
    "closest_highest": ["two_equal"],
    "capsule_x": ["capsule"],
    "inverse_rot_to_world": ["capsule", "cuboid", "far"],
    "ignore_scale": ["capsule"],
    "cuboid_farthest_face": ["cuboid", "aligned", "far", "two_equal"],
}
PART_VARIANTS = ("no_persistence", "unmirrored", "swap_dist_normal0")


@pytest.mark.parametrize("name,d,h", CASES)
def test_perturbations_are_caught(monkeypatch, name, d, h):
    monkeypatch.setattr(T, "report_margin", lambda *a, **k: None)     # (perturbed fields are no measured margins)
    sc, prev, truth = _scene(name, d, h)
    nf, pf = truth.nodes, truth.particles
    cols = CT.colliders_of(sc["colliders"], d)
    # control: the unperturbed truth, rounded to fp32 like every perturbed field below, passes the same checks
    fails = []
    CT.check_nodes("control", nf, nf.dist.astype(np.float32), nf.aff, nf.closest, fails)
    CT.check_particle_cdf("control", pf, pf.aff, pf.dist.astype(np.float32), pf.normal.astype(np.float32), fails)
    assert not fails, "\n".join(fails)
    for v, scenes in NODE_VARIANTS.items():
        if name not in scenes or (v == "closest_highest" and not T._pow2(h)) or \
                (v == "euclid_within" and name == "aligned" and not (d == 3 and T._pow2(h))):
            continue
        bad = CT.NodeField(cols, d, h, nf.cells, variant=(v,))
        fails = []
        CT.check_nodes(f"{v}", nf, bad.dist.astype(np.float32), bad.aff, bad.closest, fails)
        assert fails, f"{v} is not caught on {name} {d}D h={h}"
    for v in PART_VARIANTS:
        bad = CT.from_truth_nodes(sc["particles"].pos, h, nf, prev, variant=(v,))
        fails = []
        CT.check_particle_cdf(f"{v}", pf, bad.aff, bad.dist.astype(np.float32), bad.normal.astype(np.float32), fails)
        assert fails, f"{v} is not caught on {name} {d}D h={h}"


def test_det_edge_scene_has_decided_particles_on_both_sides(oracle_libs):
    sc = CT.det_edge()
    truth = CT.truth_of(sc)
    nf, pf = truth.nodes, truth.particles
    CT.assert_caps("det edge truth", nf, pf, part_cap=CT.DET_EDGE_CAP)
    dec = pf.reaches & ~pf.undecided
    below, above = int((dec & ~pf.ok).sum()), int((dec & pf.ok).sum())
    report_margin("det edge: decided particles below / above 1e-8", below, 20, above=above)
    assert below >= 20 and above >= 20
    o = CT._oracle_fields(sc, np.float32, np.zeros(sc["particles"].n, np.uint32))
    fails = []
    CT.check_nodes("det edge fp32 oracle", nf, o["dist"], o["aff"], o["closest"], fails)
    CT.check_particle_cdf("det edge fp32 oracle end to end", pf, o["paff"], o["pdist"], o["pnormal"], fails)
    assert not fails, "\n".join(fails)
