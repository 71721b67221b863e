"""CPU: the fp64 truth of a grid sample (tests/probe_truth.py) and its bounds are right.

- where every stencil node is present, the truth is transfer_truth.isolated's vel_g and grad on the same points;
- an fp32 numpy evaluation of the three formulas, in both summation orders (the 3^D terms one after the other; the tensor-product
  order of the step's G2P), fits the bounds on every input set of tests/test_gpu_probe.py, with the grid taken from the fp64
  transfer_truth.Grid of the scene: the bounds are never validated by the code under test;
- active_nodes is exact, bad points give all-zero records, a record scaled by 1 + 2e-3 lands outside the bounds (the weight-error term
  allows ~2e-4 of sum |v_i| at a power-of-two h near the origin)."""
import numpy as np
import pytest

import probe_truth as PT
import transfer_truth as T


def _scene_grid(name, d, h):
    sc = T.SCENES[name](d, h)
    inp = T.Inputs.of(sc["particles"])
    _, gr, _ = T.substep(inp, h, T.DT, T.GRAVITY[:d])
    cells, vm = PT.whole_block_grid(gr)
    return sc, inp, gr, cells, vm


@pytest.mark.parametrize("name,d,h", PT.CASES)
def test_truth_equals_the_isolated_g2p_truth_where_every_node_is_present(name, d, h):
    sc, inp, gr, cells, vm = _scene_grid(name, d, h)
    pos = sc["particles"].pos
    tr = PT.Truth(pos, h, cells, vm)
    assert not tr.bad.any() and (tr.active_nodes == 3 ** d).all()
    iso = T.isolated(T.Inputs.of(sc["particles"]), T.Stencil(inp, h), cells, vm[:, :d], T.DT)
    assert np.array_equal(tr.velocity, iso.vel_g) and np.array_equal(tr.gradient, iso.grad)
    assert np.array_equal(tr.b_vel, iso.b_vel_g) and np.array_equal(tr.b_grad, iso.b_grad)
    # the density is the node mass interpolated: sum w m / h^D, by hand
    st = tr.stencil
    i = gr.lookup(st.node.reshape(-1, d)).reshape(len(pos), -1)
    m32 = np.asarray(np.asarray(gr.mass, np.float32), np.float64)
    assert np.allclose(tr.density, (st.w * m32[i]).sum(1) / h ** d, rtol=1e-13, atol=0.0)


@pytest.mark.parametrize("order", ["direct", "tensor"])
@pytest.mark.parametrize("name,d,h", PT.CASES)
def test_fp32_evaluations_fit_the_bounds_on_every_point_set(name, d, h, order):
    sc, inp, gr, cells, vm = _scene_grid(name, d, h)
    fails = []
    hanging = 0
    for pname, pts in PT.probe_points(sc["particles"].pos, h, cells, seed=d):
        tr = PT.Truth(pts, h, cells, vm)
        v, g, r, a = PT.eval32(pts, h, cells, vm, order)
        PT.compare(f"fp32 numpy {order}, {name} {d}D h={h}, {pname}", tr, v, g, r, a, fails)
        assert np.array_equal(a, tr.active_nodes)
        hanging += int(((tr.active_nodes > 0) & (tr.active_nodes < 3 ** d)).sum())
    assert not fails, "\n".join(fails)
    assert hanging > 0, "no stencil hangs over the rim of the grid: the jitter does not reach it"


def test_ties_are_exact_at_a_power_of_two_cell_width():
    rng = np.random.default_rng(0)
    base = rng.uniform(-5, 5, (50, 3)).astype(np.float32)
    pts = PT.tie_points(base, 0.5, rng)
    q = pts.astype(np.float64) / 0.5
    assert (np.abs(q - np.floor(q) - 0.5) == 0.0).any(1).sum() >= len(pts) // 3 - 1
    # a point exactly on a tie has a stencil weight of exactly 0
    tr = PT.Truth(pts, 0.5, np.zeros((0, 3), np.int64), np.zeros((0, 4)))
    assert (tr.stencil.w == 0.0).any() and (tr.active_nodes == 0).all() and not tr.velocity.any()


@pytest.mark.parametrize("d", [2, 3])
def test_bad_points_and_absent_nodes(d):
    h = 0.5
    sc, inp, gr, cells, vm = _scene_grid("ties", d, h)
    pos = sc["particles"].pos[:40].copy()
    bad = pos.copy()
    vals = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    for i in range(len(bad)):
        bad[i, i % d] = vals[i % len(vals)]
    bw = PT.bw_of(d)
    last_in = (0x8000 if d == 2 else 0x400) * bw * h             # first cell of the last block inside the range, along x
    edge = np.zeros((4, d), np.float32)
    edge[:, 0] = [last_in + 1.0 * h, last_in + (bw - 1.4) * h, last_in + (bw - 0.4) * h, last_in + (bw + 1) * h]
    exp_bad = [False, True, True, True]     # associated cell 0 of the block: inside; cells BW-2.., the next block: the stencil leaves the range
    tr = PT.Truth(np.concatenate([bad, edge, pos]), h, cells, vm)
    assert tr.bad[:40].all() and list(tr.bad[40:44]) == exp_bad and not tr.bad[44:].any()
    assert not tr.velocity[:40].any() and not tr.gradient[:40].any() and not tr.density[:40].any() and not tr.active_nodes[:40].any()
    ref = PT.Truth(pos, h, cells, vm)
    assert np.array_equal(tr.velocity[44:], ref.velocity) and np.array_equal(tr.active_nodes[44:], ref.active_nodes)
    # no grid at all: everything is zero
    none = PT.Truth(pos, h, cells[:0], vm[:0])
    assert not none.velocity.any() and not none.density.any() and not none.active_nodes.any()
    # a grid that lacks one block: the stencils that reached it count fewer nodes and lose its part of the sums
    blk = cells // bw
    drop = np.all(blk == (PT.assoc_cell(pos[:1], h) // bw), axis=1)          # the block of the first point's associated cell
    part = PT.Truth(pos, h, cells[~drop], vm[~drop])
    assert (part.active_nodes <= ref.active_nodes).all() and (part.active_nodes < ref.active_nodes).any()
    fewer = part.active_nodes < ref.active_nodes
    assert np.array_equal(part.velocity[~fewer], ref.velocity[~fewer])


@pytest.mark.parametrize("d", [2, 3])
def test_perturbations_break_the_bounds(d):
    h = 0.5
    sc, inp, gr, cells, vm = _scene_grid("coordinates", d, h)
    pts = sc["particles"].pos[:60]                                            # the cluster around the origin
    tr = PT.Truth(pts, h, cells, vm)
    v, g, r, a = PT.eval32(pts, h, cells, vm, "tensor")
    fails = []
    PT.compare("clean", tr, v, g, r, a, fails)
    assert not fails
    for what, (v2, g2, r2) in dict(velocity=(v * np.float32(1 + 2e-3), g, r), gradient=(v, g * np.float32(1 + 2e-3), r),
                                   density=(v, g, r * np.float32(1 + 2e-3))).items():
        f = []
        PT.compare("perturbed", tr, v2, g2, r2, a, f)
        assert f and all(what in x for x in f), (what, f)
    f = []
    PT.compare("perturbed", tr, v, g, r, a + 1, f)
    assert f and "active_nodes" in f[0]


def test_dense_window_scatters_the_grid():
    cells = np.array([[0, 0], [1, 0], [3, 2], [-1, 5]])
    vm = np.arange(12, dtype=np.float32).reshape(4, 3) + 1
    vel, mass = PT.dense_window(cells, vm, (0, 0), (4, 3))
    assert vel.shape == (4, 3, 2) and mass.shape == (4, 3)
    assert mass[0, 0] == 3 and mass[1, 0] == 6 and mass[3, 2] == 9 and mass.sum() == 18
    assert np.array_equal(vel[3, 2], [7, 8])
