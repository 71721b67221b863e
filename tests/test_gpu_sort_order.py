"""The order the sort leaves (kernels_sort.h, launch 2), asserted directly: every active block's run goes by in-block cell and
by ascending particle id inside a cell (gpu_common.assert_canonical_order). One small scene per path of the regrouping of a
block; each scene asserts, in numpy and from the positions the sort saw, that it drives the path it is named after.

A scene is a lattice of particles at rest density (no stress) with one velocity for all of them and no gravity, so it
translates rigidly and who crosses which cell boundary in which substep is set by where the particles start. The sort of
substep k orders the state substep k - 1 left, and what it meets as "changed cell" is the motion of substep k - 1: the
preconditions compare the positions before substep k - 1 (`pos_a`) with those before substep k (`pos_b`).

The CPU twins (not marked gpu) step the same scenes with the fp32 oracle and assert the same preconditions, and show that the
helper accepts a canonical order and rejects it after one swap."""
import numpy as np
import pytest

from wgsparkl_amd.solver import Collider

from oracle.np_oracle import assoc_cell
from helpers import debug, new_data, oracle
from gpu_common import assert_canonical_order, assert_runs_canonical
from sort_truth import ARRC, BLK_ARR, H, NEWC, RUNCAP, _clump, _lexsorted_runs, _scene, facts     # (the constants: read from kernels_sort.h / layout.h)


def _lattice(lo_cell, ncells, ppc, jitter, rng, shift=0.0):
    """ppc[k] particles per cell and axis in the cells [lo_cell, lo_cell + ncells) (cell c holds x / h in [c + 0.5, c + 1.5)),
    jittered by +-jitter[k] cells; `shift`: the whole lattice moved by that much along x"""
    ax = [lo_cell[k] + 0.5 + (np.arange(ncells[k] * ppc[k]) + 0.5) / ppc[k] for k in range(len(lo_cell))]
    pos = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, len(lo_cell))
    pos = pos + rng.uniform(-1.0, 1.0, pos.shape) * np.asarray(jitter)
    pos[:, 0] += shift
    return pos * H


# ---- the scenes: name -> (scene, substeps, precondition on facts())
def _steady(dim=3, colliders=(), lo_y=8):
    rng = np.random.default_rng(5)
    if dim == 3:
        return _scene(_lattice((8, lo_y, 8), (8, 8, 4), (2, 2, 2), (0.2, 0.2, 0.2), rng), (0.05, 0.03, -0.02), colliders)
    return _scene(_lattice((16, 16), (16, 8), (4, 2), (0.1, 0.2), rng), (0.05, 0.03))


def _is_steady(f):
    assert f["changed_cell_in_block"] > 0 and f["changed_block"] > 0
    assert f["prev_run"].max() <= RUNCAP and f["per_block"].max() <= RUNCAP
    assert (f["prev_run"].max() + f["arrivals"].max()) <= RUNCAP and f["arrivals"].max() <= BLK_ARR     # the wave-parallel form
    assert 6 <= np.median(f["per_cell"]) <= 10


def _rebuild():
    rng = np.random.default_rng(6)
    pos = np.concatenate([_lattice((8, 8, 8), (8, 4, 4), (2, 2, 2), (0.2, 0.2, 0.2), rng), _clump((10.0, 10.0, 10.0), 70, rng, 0.3)])
    return _scene(pos, (0.05, 0.03, -0.02))


def _is_rebuild(f):
    assert f["per_cell"].max() > 64                                   # the smallest-key selection of next_arrival
    assert ((f["per_cell"] > ARRC) & (f["per_cell"] <= 64)).any()     # the cooperative path


CROWDED_K = 6


def _crowded():
    # two clumps that enter cell (12, 10, 9) — local (0, 2, 1) of block (3, 2, 2) — in the substep before the last: one across the
    # block's x face from block (2, 2, 2), one across a y face inside the block; 0.225 cells from the face at 0.05 cells per substep
    rng = np.random.default_rng(7)
    d = 0.05 * (CROWDED_K - 2) + 0.025
    pos = np.concatenate([_lattice((8, 8, 8), (8, 4, 4), (2, 2, 2), (0.2, 0.2, 0.2), rng),
                          _clump((12.5 - d, 11.0, 10.0), 6, rng), _clump((13.0, 10.5 - d, 10.0), 6, rng)])
    return _scene(pos, (0.05, 0.05, 0.0))


def _is_crowded(f):
    both = (f["new_same"] >= 1) & (f["new_other"] >= 1) & (f["new_same"] + f["new_other"] > NEWC)
    assert both.any()
    assert f["new_same"].max() > NEWC and f["new_other"].max() > NEWC
    assert f["arrivals"].max() <= BLK_ARR and (f["prev_run"].max() + f["arrivals"].max()) <= RUNCAP     # still the wave-parallel form


OVERFULL_K = 7


def _overfull():
    # 12 per cell in layers of six across x, no jitter along x: a whole layer crosses every face of a block in one substep
    rng = np.random.default_rng(8)
    return _scene(_lattice((8, 8, 8), (8, 4, 4), (2, 3, 2), (0.0, 0.1, 0.1), rng, shift=-0.025), (0.05, 0.0, 0.0))


def _is_overfull(f):
    assert f["arrivals"].max() > BLK_ARR
    assert f["prev_run"].max() <= RUNCAP


def _dense():
    rng = np.random.default_rng(77)
    ax = (np.arange(24, dtype=np.float64) + 0.5) * (H / 3.0) + 8.5
    pos = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return _scene(pos + rng.uniform(-0.1, 0.1, pos.shape), (0.04, 0.03, -0.02))


def _is_dense(f):
    assert f["per_block"].max() > RUNCAP and f["prev_run"].max() > RUNCAP
    assert f["changed_cell_in_block"] > 0


def _floor():
    return _steady(colliders=[Collider.cuboid((1000.0, 2.0, 1000.0), (0.0, 0.0, 0.0))], lo_y=2)


def _moving():
    return _steady(colliders=[Collider.ball(2.0, (6.0, 12.0, 10.5), linvel=(10.0, 0.0, 0.0))])


def _moved(f):
    assert f["changed_cell_in_block"] > 0 and f["changed_block"] > 0


def _some_collider_moves(sc):
    """the host's rule for the instantiation of a collider scene (host_substep.inc: summaries where a collider has a velocity or a
    mass; the whole-tile form where all are at rest)"""
    return any(np.any(np.asarray(c.linvel) != 0.0) or np.any(np.asarray(c.angvel) != 0.0) or np.any(np.asarray(c.inv_mass) != 0.0)
               or np.any(np.asarray(c.inv_inertia_local) != 0.0) for c in sc["colliders"])


def _check_instantiation(name, sc):
    if name in ("floor", "moving"):
        assert len(sc["colliders"]) > 0 and all(c.shape_type < 3 for c in sc["colliders"])      # analytic shapes: the cdf rides in the sort
        assert _some_collider_moves(sc) == (name == "moving")
    else:
        assert not sc["colliders"]


SCENES = {
    "rebuild": (_rebuild, 1, _is_rebuild),
    "steady": (_steady, 6, _is_steady),
    "crowded": (_crowded, CROWDED_K, _is_crowded),
    "overfull": (_overfull, OVERFULL_K, _is_overfull),
    "dense": (_dense, 4, _is_dense),
    "steady2d": (lambda: _steady(dim=2), 6, _is_steady),
    "floor": (_floor, 6, _moved),
    "moving": (_moving, 6, _moved),
}


def _check_on_gpu(name):
    build, k, precondition = SCENES[name]
    sc = build()
    _check_instantiation(name, sc)
    ps = sc["particles"]
    pipe, data = new_data(sc)
    poses0 = data.read_body_poses()
    pos_a, pos_b = None, ps.pos
    if k > 1:
        pipe.step(data, k - 2)
        data.sync()
        pos_a = data.read_particles().pos
        pipe.step(data, 1)
        data.sync()
        pos_b = data.read_particles().pos
    pipe.step(data, 1)
    data.sync()
    precondition(facts(pos_a, pos_b, ps.dim))
    vid, first, num, ids = assert_canonical_order(data, pos_b, ps.dim, H)
    if name == "dense":
        assert num.max() > RUNCAP, "the scene must exceed the LDS stage"
    if name in ("floor", "moving"):
        assert data.stats()["num_near_collider_blocks"] > 0
        # (the device integrates the pose of a collider the library counts as moving, and of no other)
        went = any(not np.array_equal(np.asarray(a["translation"]), np.asarray(b["translation"])) for a, b in zip(poses0, data.read_body_poses()))
        assert went == (name == "moving")
    # (by block: where a block's run lies in `ids` goes by its physical id, which the table hands out in the order of arrival)
    return {tuple(v): ids[f:f + n].tolist() for v, f, n in zip(vid.tolist(), first.tolist(), num.tolist())}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_sort_leaves_the_canonical_order(hip_libs, name):
    _check_on_gpu(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["steady", "crowded"])
def test_insertion_sort_fallback_leaves_the_same_order(hip_libs, monkeypatch, name):
    runs = _check_on_gpu(name)
    with debug(monkeypatch, "CELL_INSERTION_SORT"):
        assert _check_on_gpu(name) == runs


# ---- CPU twins
@pytest.mark.parametrize("name", list(SCENES))
def test_scene_drives_its_path_on_the_oracle(oracle_libs, name):
    build, k, precondition = SCENES[name]
    sc = build()
    _check_instantiation(name, sc)
    ps = sc["particles"]
    assert ps.n <= 14000
    st = oracle(ps.dim, np.float32).new_state(ps, sc["params"], sc["colliders"], sc["cell_width"], sc["grid_capacity"], sc["model"])
    pos_a, pos_b = None, ps.pos
    if k > 1:
        st.step(k - 2)
        pos_a = st.arr["pos"].copy()
        st.step(1)
        pos_b = st.arr["pos"].copy()
    st.step(1)
    assert not st.overflow
    precondition(facts(pos_a, pos_b, ps.dim))


@pytest.mark.parametrize("dim", [2, 3])
def test_helper_accepts_a_canonical_order_and_rejects_one_swap(dim):
    pos = SCENES["steady" if dim == 3 else "steady2d"][0]()["particles"].pos
    vid, first, num, ids = _lexsorted_runs(pos, dim)
    assert_runs_canonical(vid, first, num, ids, pos, dim, H)
    cell = assoc_cell(pos, H)
    same = next(i for i in range(len(ids) - 1) if (cell[ids[i]] == cell[ids[i + 1]]).all())
    other = next(i for i in range(len(ids) - 1) if (cell[ids[i]] != cell[ids[i + 1]]).any() and i + 1 < first[1])
    for i in (same, other):        # one swap inside a cell; one across two cells of a block
        bad = ids.copy()
        bad[[i, i + 1]] = bad[[i + 1, i]]
        with pytest.raises(AssertionError):
            assert_runs_canonical(vid, first, num, bad, pos, dim, H)
    dup = ids.copy()
    dup[0] = dup[1]
    with pytest.raises(AssertionError):
        assert_runs_canonical(vid, first, num, dup, pos, dim, H)
