"""-m "not gpu": the domain-wall rule as tests/wall_truth.py states it — what tests/test_gpu_walls.py holds the HIP kernel to.
Membership at and around a plane, what friction == 0 may write, SEPARATE against SLIP, the order of the faces at a corner, the
limit of a huge friction, and the truth substep with walls."""
import numpy as np
import pytest

import transfer_truth as T
import wall_truth as W


def _nodes(d, lo=-8, hi=9, seed=0):
    ax = [np.arange(lo, hi)] * d
    cells = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, d)
    rng = np.random.default_rng(seed)
    vel = rng.normal(0.0, 3.0, cells.shape).astype(np.float32)
    vel[rng.random(len(vel)) < 0.05] = 0.0
    vel[rng.random(len(vel)) < 0.05, 0] = np.float32(-0.0)
    return cells, vel


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("plane", [5, 0, -3])
def test_membership_at_and_around_the_plane(d, plane):
    cells, vel = _nodes(d)
    for k in range(d):
        for side in (0, 1):
            walls = [None] * (2 * d)
            walls[2 * k + side] = (W.STICKY, 0.0, plane)
            out = W.apply(cells, vel, walls)
            c = cells[:, k]
            for at, hit in ((plane - 1, side == 0), (plane, True), (plane + 1, side == 1)):
                sel = c == at
                assert sel.any()
                if hit:
                    assert not out[sel].any()
                else:
                    assert np.array_equal(W.bits(out[sel]), W.bits(vel[sel]))
            assert np.array_equal(W.members(cells, walls)[:, 2 * k + side], c >= plane if side else c <= plane)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("typ", [W.STICKY, W.SLIP, W.SEPARATE])
def test_frictionless_rules_are_idempotent_and_write_only_zeros(d, typ):
    cells, vel = _nodes(d, seed=1)
    walls = [(typ, 0.0, -3 if f % 2 == 0 else 4) for f in range(2 * d)]
    once = W.apply(cells, vel, walls)
    b0, b1 = W.bits(vel), W.bits(once)              # (bits: also asserts that the result is an fp32 array)
    changed = b0 != b1
    assert changed.any()
    assert np.all((b1[changed] & 0x7fffffff) == 0), "a frictionless face wrote something other than a zero"
    assert np.array_equal(W.bits(W.apply(cells, once, walls)), b1)
    assert not changed[~W.members(cells, walls).any(1)].any(), "a node outside every face changed"


@pytest.mark.parametrize("d", [2, 3])
def test_separate_is_slip_where_the_node_moves_into_the_wall_and_the_identity_elsewhere(d):
    cells, vel = _nodes(d, seed=2)
    for f in range(2 * d):
        for fr in (0.0, 0.4):
            mk = lambda typ: [(typ, fr, 2) if g == f else None for g in range(2 * d)]
            sep, slip = W.apply(cells, vel, mk(W.SEPARATE)), W.apply(cells, vel, mk(W.SLIP))
            k = f >> 1
            vn = vel[:, k].astype(np.float64) if f & 1 else -vel[:, k].astype(np.float64)
            into = W.members(cells, mk(W.SLIP))[:, f] & (vn > 0)
            assert into.any() and (~into).any()
            assert np.array_equal(sep[into], slip[into])
            assert np.array_equal(W.bits(sep[~into]), W.bits(vel[~into]))


def test_a_corner_node_takes_the_faces_in_array_order():
    """Friction on two faces: the first face's friction is computed from the normal component the second face has not removed yet,
    so the order matters, and the order is that of the array."""
    cells = np.array([[0, 0]])
    v = np.array([[-3.0, -4.0]], np.float32)
    walls = [(W.SLIP, 0.5, 0), None, (W.SLIP, 0.5, 0), None]
    # axis 0 low first: vn = 3, vt = |-4| = 4 -> v = (0, -4 (1 - 1.5 / 4)) = (0, -2.5); then axis 1 low: vn = 2.5, vt = 0 -> (0, 0)
    assert np.array_equal(W.apply(cells, v, walls), [[0.0, 0.0]])
    one = W.apply(cells, v, [walls[0], None, None, None])
    assert np.array_equal(one, [[0.0, -2.5]])
    # sticky behind slip is sticky; a face that does not hold the node does nothing
    assert np.array_equal(W.apply(cells, v, [walls[0], None, (W.STICKY, 0.0, 0), None]), [[0.0, 0.0]])
    assert np.array_equal(W.apply(cells, v, [walls[0], (W.SLIP, 0.5, 1), None, None]), one)
    # a case where the order shows in the result: 3D, the two frictional faces share a tangential axis
    c3 = np.array([[0, 0, 0]])
    v3 = np.array([[-1.0, -2.0, 8.0]], np.float32)
    a = W.apply(c3, v3, [(W.SLIP, 1.0, 0), None, (W.SLIP, 1.0, 0), None, None, None])
    # x first: vt = |(-2, 8)|, s = 1 - 1 / sqrt(68); then y: vn = 2 s, vt = 8 s -> z = 8 s (1 - 2 s / (8 s)) = 6 s
    s = 1.0 - 1.0 / np.sqrt(68.0)
    assert np.allclose(a, [[0.0, 0.0, 6.0 * s]], rtol=1e-15)
    # y first (what the other order would give): vt = |(-1, 8)|, s' = 1 - 2 / sqrt(65); then x: z = 8 s' (1 - 1 / 8) = 7 s'
    assert abs(7.0 * (1.0 - 2.0 / np.sqrt(65.0)) - a[0, 2]) > 1e-3


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("typ", [W.SLIP, W.SEPARATE])
def test_a_huge_friction_stops_every_node_that_moves_into_the_wall(d, typ):
    cells, vel = _nodes(d, seed=3)
    walls = [(typ, 1.0e6, 0) if f == 2 else None for f in range(2 * d)]      # the low face of axis 1
    out = W.apply(cells, vel, walls)
    into = (cells[:, 1] <= 0) & (-vel[:, 1].astype(np.float64) > 1e-3)
    assert into.any()
    assert not out[into].any()


@pytest.mark.parametrize("d,h", [(2, 1.0), (3, 0.3)])
def test_truth_substep_with_walls(d, h):
    """Grid, then the rule, then Particles: without walls it is transfer_truth.substep; with a sticky face every particle whose
    whole stencil lies inside it stands still; with a slip floor no particle whose whole stencil lies inside it moves into the floor."""
    rng = np.random.default_rng(5)
    sc = T._finish(rng.uniform(2.0 * h, 14.0 * h, (800, d)), h, rng, vel_scale=4.0 * h)
    inp = T.Inputs.of(sc["particles"])
    none = [None] * (2 * d)
    _, gr0, pt0 = T.substep(inp, h, T.DT, T.GRAVITY[:d])
    st, gr, vw, bw, pt = W.substep(inp, h, T.DT, T.GRAVITY[:d], none)
    assert np.array_equal(vw, gr0.vel) and np.array_equal(pt.x, pt0.x) and np.array_equal(pt.F, pt0.F) and np.array_equal(pt.b_vel, pt0.b_vel)
    plane = 6
    for typ in (W.STICKY, W.SLIP):
        walls = list(none)
        walls[2] = (typ, 0.0, plane)
        st, gr, vw, bw, pt = W.substep(inp, h, T.DT, T.GRAVITY[:d], walls)
        deep = st.node[:, :, 1].max(1) <= plane
        assert deep.sum() > 20
        if typ == W.STICKY:
            assert not pt.vel[deep].any() and np.array_equal(pt.x[deep], inp.x[deep]) and np.array_equal(pt.F[deep], inp.F[deep])
        else:
            assert not pt.vel[deep, 1].any() and pt.vel[deep, 0].any()
        free = st.node[:, :, 1].min(1) > plane
        assert np.array_equal(pt.x[free], pt0.x[free])
        assert np.all(bw >= 0) and np.array_equal(bw, gr.bounds()[1])       # friction 0: the rule adds nothing to a node's bound
    walls = list(none)
    walls[2] = (W.SLIP, 0.5, plane)
    _, gr, vw, bw, _ = W.substep(inp, h, T.DT, T.GRAVITY[:d], walls)
    m = W.members(gr.cells, walls)[:, 2]
    assert np.allclose(bw[m], 1.5 * gr.bounds()[1][m] + W.C_WALL * T.U32 * np.linalg.norm(gr.vel[m], axis=1), rtol=1e-14)
    assert np.array_equal(bw[~m], gr.bounds()[1][~m])
